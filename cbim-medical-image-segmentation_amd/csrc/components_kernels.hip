// components_kernels.hip — connected components of a uint8 label map [D, H, W] and the clean-up built on them ("keep the largest
// component of each organ, drop specks below N voxels").  Two voxels are connected iff they are neighbours under the chosen
// connectivity (6 / 18 / 26) AND carry the same non-zero value, so one pass labels every class at once.
//
// Union-find over int32 parent[N] in which THE SMALLER LINEAR INDEX WINS: a link always points from a voxel to a smaller index of
// the same component, so the root of a component is its first voxel in raster order.  The final partition and every root are
// unique: they do not depend on the order in which the atomics land, and every later stage is integer arithmetic on them, so all
// outputs are bitwise reproducible.
//
//   k_cc_tile     one workgroup per 8 x 8 x 32 tile: parent = own index (-1 for background), merge inside the tile in LDS, write
//                 the tile-local roots as global linear indices
//   k_cc_border   voxels on tile faces: union with the backward neighbours (3 / 9 / 13 of them) that lie in ANOTHER tile, global
//                 atomicMin
//   k_cc_flatten  parent[i] = find(i)
//   k_cc_sizes    size[root] += 1, runs of equal roots inside a wave aggregated to one atomic
//   k_cc_best     best[class] = max over the class's roots of (size << 32) | (0xFFFFFFFF - root): the largest component, ties to
//                 the smaller root; reduced in LDS first
//   k_cc_filter   out = keep ? in : 0 from size[root], best[class] and the two 256-entry tables
//   k_cc_count / k_cc_scan / k_cc_rank / k_cc_comp   component ids 1..n in raster order of the roots (exclusive prefix count of
//                 parent[i] == i)
//
// Lock-free throughout: no workgroup ever waits for a value another one must write.  Visibility: a link is only ever created by
// the atomicMin itself, and what the loops READ may be stale without harm, because parents only decrease and stay inside the
// component: a stale parent is still an ancestor.  The border pass, the only one in which workgroups touch each other's entries,
// nevertheless reads parent with relaxed agent-scope loads, and its union loop ends only on the atomic's return value or on two
// such loads agreeing.  Every other stage is its own launch and sees everything the launches before it wrote.
#include "atomics_compat.h"

namespace cbim {

static constexpr int CC_T = 256;
static constexpr int CC_TX = 32, CC_TY = 8, CC_TZ = 8, CC_TV = CC_TX * CC_TY * CC_TZ;
static constexpr int CC_CHUNK = 2048;   // voxels per workgroup of the numbering kernels

struct CcLdsLoad { static __device__ __forceinline__ int ld(const int* p) { return *(const volatile int*)p; } };
struct CcPlainLoad { static __device__ __forceinline__ int ld(const int* p) { return *(const volatile int*)p; } };
struct CcAgentLoad { static __device__ __forceinline__ int ld(const int* p) { return load_agent(p); } };

template <typename LD>
__device__ __forceinline__ int cc_find(const int* p, int x) {
  // Termination: the loop goes on only while the value read is a smaller non-negative index, so x strictly decreases and the
  // loop ends after at most x steps whatever other threads write meanwhile.
  while (true) {
    const int q = LD::ld(p + x);
    if (q >= x || q < 0) return x;
    x = q;
  }
}

template <typename LD>
__device__ __forceinline__ void cc_union(int* p, int a, int b) {
  // Termination: an iteration either returns or replaces the larger of (a, b) by the atomic's previous value old < hi while
  // the other one does not grow (find only descends), so a + b >= 0 strictly decreases: the loop ends on any interleaving.
  // It never waits: every iteration makes its own progress from what it has just read.
  while (true) {
    a = cc_find<LD>(p, a);
    b = cc_find<LD>(p, b);
    if (a == b) return;                    // one common ancestor: already one set
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(p + hi, lo);
    if (old == hi) return;                 // hi was a root when the atomic landed; it now hangs under lo
    a = old;                               // hi already hung under old < hi (and now under min(old, lo)):
    b = lo;                                // what is left to join is old's set with lo's
  }
}

// the backward neighbours (those before the voxel in raster order) under connectivity norm m = 1 / 2 / 3 (6 / 18 / 26)
#define CC_FOR_BACKWARD(m, dz, dy, dx)                                                         \
  for (int dz = -1; dz <= 0; ++dz)                                                             \
    for (int dy = -1; dy <= (dz ? 1 : 0); ++dy)                                                \
      for (int dx = -1; dx <= ((dz || dy) ? 1 : -1); ++dx)                                     \
        if ((dz != 0) + (dy != 0) + (dx != 0) <= (m))

struct CcTile { int x0, y0, z0; };
__device__ __forceinline__ CcTile cc_tile_of(int tiles_x, int tiles_y) {
  const int t = blockIdx.x;
  CcTile r;
  r.x0 = (t % tiles_x) * CC_TX;
  r.y0 = ((t / tiles_x) % tiles_y) * CC_TY;
  r.z0 = (t / (tiles_x * tiles_y)) * CC_TZ;
  return r;
}

__global__ void __launch_bounds__(CC_T) k_cc_tile(const uint8_t* __restrict__ lab, int D, int H, int W, int m, int tiles_x,
                                                  int tiles_y, int* __restrict__ parent) {
  __shared__ int lp[CC_TV];
  __shared__ uint8_t sl[CC_TV];
  const CcTile t = cc_tile_of(tiles_x, tiles_y);
  const int lx = threadIdx.x & (CC_TX - 1), ly = threadIdx.x / CC_TX;
  const int x = t.x0 + lx, y = t.y0 + ly;
  const bool inxy = x < W && y < H;
  for (int lz = 0; lz < CC_TZ; ++lz) {
    const int z = t.z0 + lz, l = (lz * CC_TY + ly) * CC_TX + lx;
    const uint8_t v = (inxy && z < D) ? lab[((size_t)z * H + y) * W + x] : (uint8_t)0;
    sl[l] = v;
    lp[l] = v ? l : -1;
  }
  __syncthreads();
  for (int lz = 0; lz < CC_TZ; ++lz) {
    const int l = (lz * CC_TY + ly) * CC_TX + lx;
    const uint8_t v = sl[l];
    if (!v) continue;
    CC_FOR_BACKWARD(m, dz, dy, dx) {
      const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
      if (nz < 0 || ny < 0 || ny >= CC_TY || nx < 0 || nx >= CC_TX) continue;
      const int j = (nz * CC_TY + ny) * CC_TX + nx;
      if (sl[j] == v) cc_union<CcLdsLoad>(lp, l, j);
    }
  }
  __syncthreads();
  for (int lz = 0; lz < CC_TZ; ++lz) {
    const int z = t.z0 + lz, l = (lz * CC_TY + ly) * CC_TX + lx;
    if (!inxy || z >= D) continue;
    int g = -1;
    if (sl[l]) {   // local order == raster order inside a tile, so the local root is the tile's first voxel of the component
      const int r = cc_find<CcLdsLoad>(lp, l);
      const int rx = r & (CC_TX - 1), ry = (r / CC_TX) & (CC_TY - 1), rz = r / (CC_TX * CC_TY);
      g = (int)(((int64_t)(t.z0 + rz) * H + (t.y0 + ry)) * W + (t.x0 + rx));
    }
    parent[((size_t)z * H + y) * W + x] = g;
  }
}

__global__ void __launch_bounds__(CC_T) k_cc_border(const uint8_t* __restrict__ lab, int D, int H, int W, int m, int tiles_x,
                                                    int tiles_y, int* parent) {
  const CcTile t = cc_tile_of(tiles_x, tiles_y);
  const int lx = threadIdx.x & (CC_TX - 1), ly = threadIdx.x / CC_TX;
  const int x = t.x0 + lx, y = t.y0 + ly;
  if (x >= W || y >= H) return;
  for (int lz = 0; lz < CC_TZ; ++lz) {
    const int z = t.z0 + lz;
    if (z >= D) break;
    if (!(lz == 0 || ly == 0 || ly == CC_TY - 1 || lx == 0 || lx == CC_TX - 1)) continue;
    const int g = (int)(((int64_t)z * H + y) * W + x);
    const uint8_t v = lab[g];
    if (!v) continue;
    CC_FOR_BACKWARD(m, dz, dy, dx) {
      const int nlz = lz + dz, nly = ly + dy, nlx = lx + dx;
      if (!(nlz < 0 || nly < 0 || nly >= CC_TY || nlx < 0 || nlx >= CC_TX)) continue;   // same tile: k_cc_tile joined them
      const int nz = z + dz, ny = y + dy, nx = x + dx;
      if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
      const int j = (int)(((int64_t)nz * H + ny) * W + nx);
      if (lab[j] == v) cc_union<CcAgentLoad>(parent, g, j);
    }
  }
}

__global__ void __launch_bounds__(CC_T) k_cc_flatten(int* parent, int64_t N) {
  // concurrent writers only ever replace an ancestor by the root, so a racing read still yields an ancestor
  for (int64_t i = (int64_t)blockIdx.x * CC_T + threadIdx.x; i < N; i += (int64_t)gridDim.x * CC_T) {
    if (CcPlainLoad::ld(parent + i) < 0) continue;
    parent[i] = cc_find<CcPlainLoad>(parent, (int)i);
  }
}

__global__ void __launch_bounds__(CC_T) k_cc_zero(int* __restrict__ size, int64_t N, unsigned long long* __restrict__ best) {
  for (int64_t i = (int64_t)blockIdx.x * CC_T + threadIdx.x; i < N; i += (int64_t)gridDim.x * CC_T) size[i] = 0;
  if (blockIdx.x == 0) best[threadIdx.x] = 0ull;   // CC_T == 256 classes
}

__global__ void __launch_bounds__(CC_T) k_cc_sizes(const int* __restrict__ parent, int64_t N, int* __restrict__ size) {
  const int lane = threadIdx.x & 63;
  // the trip count is uniform over the workgroup: every lane takes part in the shuffle and the ballot
  for (int64_t base = (int64_t)blockIdx.x * CC_T; base < N; base += (int64_t)gridDim.x * CC_T) {
    const int64_t i = base + threadIdx.x;
    const int r = i < N ? parent[i] : -1;
    const int prev = __shfl(r, (lane + 63) & 63, 64);
    const unsigned long long heads = wave_ballot(lane == 0 || r != prev);
    if (r >= 0 && (lane == 0 || r != prev)) {     // first lane of a run of equal roots adds the run's length
      const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
      atomicAdd(size + r, len);
    }
  }
}

__global__ void __launch_bounds__(CC_T) k_cc_best(const uint8_t* __restrict__ lab, const int* __restrict__ parent,
                                                  const int* __restrict__ size, int64_t N, unsigned long long* __restrict__ best) {
  __shared__ unsigned long long sb[256];
  sb[threadIdx.x] = 0ull;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * CC_T + threadIdx.x; i < N; i += (int64_t)gridDim.x * CC_T) {
    if (parent[i] != (int)i) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)size[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    atomicMax(sb + lab[i], key);
  }
  __syncthreads();
  if (sb[threadIdx.x]) atomicMax(best + threadIdx.x, sb[threadIdx.x]);
}

__global__ void __launch_bounds__(CC_T) k_cc_filter(const uint8_t* lab, const int* __restrict__ parent, const int* __restrict__ size,
                                                    const unsigned long long* __restrict__ best, const uint8_t* __restrict__ keep_largest,
                                                    const int* __restrict__ min_size, uint8_t* out, int64_t N) {
  __shared__ int s_best[256], s_min[256];
  __shared__ uint8_t s_kl[256];
  s_best[threadIdx.x] = (int)(0xFFFFFFFFu - (unsigned)(best[threadIdx.x] & 0xFFFFFFFFull));   // -1 for an absent class
  s_min[threadIdx.x] = min_size[threadIdx.x];
  s_kl[threadIdx.x] = keep_largest[threadIdx.x];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * CC_T + threadIdx.x; i < N; i += (int64_t)gridDim.x * CC_T) {
    const uint8_t c = lab[i];     // out may alias lab: each voxel is read, then written, by one thread
    bool keep = c != 0;
    if (keep && (s_kl[c] || s_min[c] > 1)) {
      const int r = parent[i];
      keep = r >= 0 && (!s_kl[c] || r == s_best[c]) && size[r] >= s_min[c];
    }
    out[i] = keep ? c : (uint8_t)0;
  }
}

// ---- numbering: ids 1..n in raster order of the roots --------------------------------------------------------------------
__global__ void __launch_bounds__(CC_T) k_cc_count(const int* __restrict__ parent, int64_t N, int* __restrict__ counts) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * CC_CHUNK;
  int mine = 0;
  for (int k = 0; k < CC_CHUNK / CC_T; ++k) {
    const int64_t i = base + k * CC_T + threadIdx.x;
    mine += (i < N && parent[i] == (int)i) ? 1 : 0;
  }
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_n;
}

// one workgroup: counts[nb] -> exclusive prefix in place, the total into *n_out
__global__ void __launch_bounds__(CC_T) k_cc_scan(int* __restrict__ counts, int nb, int* __restrict__ n_out) {
  __shared__ int s[CC_T];
  const int seg = (nb + CC_T - 1) / CC_T;
  const int64_t b0 = (int64_t)threadIdx.x * seg;
  const int lo = (int)(b0 < nb ? b0 : nb), hi = (int)(b0 + seg < nb ? b0 + seg : nb);
  int sum = 0;
  for (int b = lo; b < hi; ++b) sum += counts[b];
  s[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < CC_T; ++k) { const int v = s[k]; s[k] = run; run += v; }
    *n_out = run;
  }
  __syncthreads();
  int run = s[threadIdx.x];
  for (int b = lo; b < hi; ++b) { const int v = counts[b]; counts[b] = run; run += v; }
}

__global__ void __launch_bounds__(CC_T) k_cc_rank(const int* __restrict__ parent, int64_t N, const int* __restrict__ offsets,
                                                  int* __restrict__ comp) {
  __shared__ int wt[CC_T / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * CC_CHUNK;
  int run = offsets[blockIdx.x];
  for (int k = 0; k < CC_CHUNK / CC_T; ++k) {     // uniform trip count: every lane takes part in the ballot and the barriers
    const int64_t i = base + k * CC_T + threadIdx.x;
    const bool root = i < N && parent[i] == (int)i;
    const unsigned long long bal = wave_ballot(root);
    if (lane == 0) wt[w] = __builtin_popcountll(bal);
    __syncthreads();
    int before = 0, all = 0;
    for (int q = 0; q < CC_T / 64; ++q) { before += q < w ? wt[q] : 0; all += wt[q]; }
    if (root) comp[i] = run + before + __builtin_popcountll(bal & ((1ull << lane) - 1ull)) + 1;
    run += all;
    __syncthreads();
  }
}

// after k_cc_rank wrote the ids of the roots: every other voxel takes its root's id, background 0 (roots are not touched here)
__global__ void __launch_bounds__(CC_T) k_cc_comp(const int* __restrict__ parent, int64_t N, int* comp) {
  for (int64_t i = (int64_t)blockIdx.x * CC_T + threadIdx.x; i < N; i += (int64_t)gridDim.x * CC_T) {
    const int r = parent[i];
    if (r < 0) comp[i] = 0;
    else if (r != (int)i) comp[i] = comp[r];
  }
}

static inline int cc_grid(int64_t items, int64_t per_block, int64_t cap) {
  int64_t b = (items + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// N = D * H * W, or 0 when a dimension is not positive or the volume has 2^31 voxels or more (indices are int32)
static inline int64_t cc_voxels(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return 0;
  const int64_t N = (int64_t)D * H * W;
  return N >= ((int64_t)1 << 31) ? 0 : N;
}

static inline bool cc_aligned(const void* p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace cbim

using namespace cbim;

#define CC_VOLUME(what)                                                                                                   \
  const int64_t N = cc_voxels(D, H, W);                                                                                   \
  CBIM_CHECK(N > 0, CBIM_EINVAL, what ": volume [%d,%d,%d] is empty or has 2^31 voxels or more (indices are int32)", D, H, W)

extern "C" int64_t cbim_components_workspace_bytes(int D, int H, int W) {
  CC_VOLUME("components_workspace_bytes");
  const int64_t nb = (N + CC_CHUNK - 1) / CC_CHUNK;
  return (nb * (int64_t)sizeof(int) + 15) / 16 * 16;
}

extern "C" int cbim_components_label(const uint8_t* labels, int D, int H, int W, int connectivity, int32_t* parent, void* stream) {
  CC_VOLUME("components_label");
  CBIM_CHECK(connectivity == 6 || connectivity == 18 || connectivity == 26, CBIM_EINVAL,
             "components_label: connectivity %d is not 6, 18 or 26", connectivity);
  CBIM_CHECK(labels && cc_aligned(parent, 4), CBIM_EINVAL, "components_label: null or misaligned pointer");
  const int m = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
  const int tiles_x = (W + CC_TX - 1) / CC_TX, tiles_y = (H + CC_TY - 1) / CC_TY, tiles_z = (D + CC_TZ - 1) / CC_TZ;
  const int64_t tiles = (int64_t)tiles_x * tiles_y * tiles_z;     // < 2^31 / 1: at most one tile per voxel
  hipStream_t st = (hipStream_t)stream;
  CBIM_LAUNCH(k_cc_tile, dim3((unsigned)tiles), dim3(CC_T), 0, st, labels, D, H, W, m, tiles_x, tiles_y, parent);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  if (tiles > 1) {
    CBIM_LAUNCH(k_cc_border, dim3((unsigned)tiles), dim3(CC_T), 0, st, labels, D, H, W, m, tiles_x, tiles_y, parent);
    if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
    CBIM_LAUNCH(k_cc_flatten, dim3(cc_grid(N, CC_T * 4, 16384)), dim3(CC_T), 0, st, parent, N);
    if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  }
  return CBIM_OK;
}

extern "C" int cbim_components_sizes(const uint8_t* labels, const int32_t* parent, int D, int H, int W, int32_t* size,
                                     uint64_t* best, void* stream) {
  CC_VOLUME("components_sizes");
  CBIM_CHECK(labels && cc_aligned(parent, 4) && cc_aligned(size, 4) && cc_aligned(best, 8), CBIM_EINVAL,
             "components_sizes: null or misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* b = (unsigned long long*)best;
  CBIM_LAUNCH(k_cc_zero, dim3(cc_grid(N, CC_T * 4, 16384)), dim3(CC_T), 0, st, size, N, b);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH(k_cc_sizes, dim3(cc_grid(N, CC_T * 4, 16384)), dim3(CC_T), 0, st, parent, N, size);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH(k_cc_best, dim3(cc_grid(N, CC_T * 16, 4096)), dim3(CC_T), 0, st, labels, parent, (const int*)size, N, b);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_components_filter(const uint8_t* labels, const int32_t* parent, const int32_t* size, const uint64_t* best,
                                      const uint8_t* keep_largest, const int32_t* min_size, uint8_t* out, int64_t N, void* stream) {
  CBIM_CHECK(N >= 1 && N < ((int64_t)1 << 31), CBIM_EINVAL, "components_filter: %lld voxels (1 .. 2^31 - 1)", (long long)N);
  CBIM_CHECK(labels && out && keep_largest && cc_aligned(parent, 4) && cc_aligned(size, 4) && cc_aligned(best, 8) &&
                 cc_aligned(min_size, 4), CBIM_EINVAL, "components_filter: null or misaligned pointer");
  CBIM_LAUNCH(k_cc_filter, dim3(cc_grid(N, CC_T * 4, 16384)), dim3(CC_T), 0, (hipStream_t)stream, labels, parent, size,
              (const unsigned long long*)best, keep_largest, min_size, out, N);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_components_number(const int32_t* parent, int D, int H, int W, int32_t* comp, int32_t* n_out, void* scratch,
                                      void* stream) {
  CC_VOLUME("components_number");
  CBIM_CHECK(cc_aligned(parent, 4) && cc_aligned(comp, 4) && cc_aligned(n_out, 4) && cc_aligned(scratch, 4), CBIM_EINVAL,
             "components_number: null or misaligned pointer");
  const int nb = (int)((N + CC_CHUNK - 1) / CC_CHUNK);
  hipStream_t st = (hipStream_t)stream;
  int* counts = (int*)scratch;
  CBIM_LAUNCH(k_cc_count, dim3(nb), dim3(CC_T), 0, st, parent, N, counts);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH(k_cc_scan, dim3(1), dim3(CC_T), 0, st, counts, nb, n_out);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH(k_cc_rank, dim3(nb), dim3(CC_T), 0, st, parent, N, (const int*)counts, comp);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH(k_cc_comp, dim3(cc_grid(N, CC_T * 4, 16384)), dim3(CC_T), 0, st, parent, N, comp);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

CBIM_DEFINE_WARM(components)
