// surface_kernels.hip — surface-distance metrics (ASD / HD95) of the evaluation loop: the reference's
// metric/metrics.py compute_surface_distances (bounding box, 2x2x2 neighbour codes, exact Euclidean distance transform of
// each surface map, distance + code per surface point) for every foreground class of two label volumes.
//
//   k_surface_scan      one pass over the corner points of both volumes: per class the box of its surface points (which IS the
//                       reference's padded bounding-box crop of gt | pred) and the number of surface points of each mask
//   k_neighbour_codes   uint8 code maps of gt and pred over every present class's box, class on blockIdx.y
//   k_edt_x             first EDT axis (x, contiguous): nearest surface point of the line, |dx| as int16
//   k_edt_minplus<2>    second axis (y): out[i] = min_j (s1 (i-j))^2 + (s2 dx[j])^2, brute force in float64 over the line,
//                       staged in LDS in tiles of 128 candidates x 32 columns; carries (|dy|, |dx|) of the winner
//   k_edt_minplus<3>    third axis (z), evaluated only at surface points of the OTHER mask; finishes the distance from the
//                       integer offsets in scipy's order sqrt(((dz s0)^2 + (dy s1)^2) + (dx s2)^2) and appends (distance,
//                       own code) to that mask's list (one global atomic per workgroup and 32-row chunk)
// The minimum over a line is taken by comparison only, so it is exact whatever the spacing; ties pick offsets of equal length.
#include "cbim_common.h"
#include "gfx950_prims.h"

#include <limits.h>

namespace cbim {

static constexpr int SF_T = 256;
static constexpr int SF_NONE16 = 32767;       // "no surface point in this line" (k_edt_x); box extents stay below it
static constexpr int MP_TX = 32, MP_TY = 8, MP_R = 4, MP_IC = MP_TY * MP_R, MP_JT = 128;

// labels of the 8 voxels around corner point (z, y, x): lab[4a + 2b + c] = voxel (z-1+a, y-1+b, x-1+c), -1 outside the
// volume; bit 128 >> k of the neighbour code belongs to lab[k] (scipy centres the 2x2x2 correlation kernel at index 1)
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ v, int D, int H, int W, int z, int y, int x, int lab[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int zz = z - 1 + (k >> 2), yy = y - 1 + ((k >> 1) & 1), xx = x - 1 + (k & 1);
    const bool in = zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W;
    lab[k] = in ? (int)v[((size_t)zz * H + yy) * W + xx] : -1;
  }
}
__device__ __forceinline__ int code_of(const int lab[8], int c) {
  int code = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) code |= (lab[k] == c) ? (128 >> k) : 0;
  return code;
}
__device__ __forceinline__ bool is_surface(int code) { return code != 0 && code != 255; }

// While the scan runs, the box fields are unsigned maxima (the one integer atomic every build of these sources has for both
// LDS and global memory): field k < 3 holds INT_MAX - min, field 3 <= k < 6 holds max + 1, 0 = no surface point yet.
// k_surface_box_decode turns them into the (min | INT_MAX, max | -1) the ABI documents.
__global__ void __launch_bounds__(SF_T) k_surface_box_decode(int* __restrict__ box, int n) {
  for (int i = blockIdx.x * SF_T + threadIdx.x; i < n; i += gridDim.x * SF_T) {
    const int k = i & 7;
    if (k < 3) box[i] = INT_MAX - box[i];
    else if (k < 6) box[i] = box[i] - 1;
  }
}
__global__ void __launch_bounds__(SF_T) k_surface_zero(int* __restrict__ p, int n) {
  for (int i = blockIdx.x * SF_T + threadIdx.x; i < n; i += gridDim.x * SF_T) p[i] = 0;
}

// every foreground class that is among the 8 labels of a corner point without filling all 8 has a surface point there
__device__ __forceinline__ void scan_point(const int lab[8], int m, int C, int z, int y, int x, int* sh) {
  bool same = true;
#pragma unroll
  for (int k = 1; k < 8; ++k) same = same && lab[k] == lab[0];
  if (same) return;
  for (int k = 0; k < 8; ++k) {
    const int c = lab[k];
    if (c < 1 || c >= C) continue;
    bool seen = false;
    for (int q = 0; q < k; ++q) seen = seen || lab[q] == c;
    if (seen) continue;
    int* b = sh + c * 8;
    unsigned* u = (unsigned*)b;
    atomicMax(u + 0, (unsigned)(INT_MAX - z)); atomicMax(u + 1, (unsigned)(INT_MAX - y)); atomicMax(u + 2, (unsigned)(INT_MAX - x));
    atomicMax(u + 3, (unsigned)(z + 1)); atomicMax(u + 4, (unsigned)(y + 1)); atomicMax(u + 5, (unsigned)(x + 1));
    atomicAdd(b + 6 + m, 1);
  }
}

template <typename TP, typename TG>
__global__ void __launch_bounds__(SF_T) k_surface_scan(const TP* __restrict__ pred, const TG* __restrict__ gt, int D, int H, int W,
                                                       int C, int* __restrict__ box) {
  CBIM_DYN_SMEM(raw);
  int* sh = (int*)raw;   // [C][8]
  for (int i = threadIdx.x; i < C * 8; i += SF_T) sh[i] = 0;
  __syncthreads();
  const int64_t total = (int64_t)(D + 1) * (H + 1) * (W + 1);
  for (int64_t i = (int64_t)blockIdx.x * SF_T + threadIdx.x; i < total; i += (int64_t)gridDim.x * SF_T) {
    const int x = (int)(i % (W + 1)), y = (int)((i / (W + 1)) % (H + 1)), z = (int)(i / ((int64_t)(W + 1) * (H + 1)));
    int lab[8];
    load8(gt, D, H, W, z, y, x, lab);
    scan_point(lab, 0, C, z, y, x, sh);
    load8(pred, D, H, W, z, y, x, lab);
    scan_point(lab, 1, C, z, y, x, sh);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * 8; i += SF_T) {      // integer atomics: exact, order-independent
    const int k = i & 7, v = sh[i];
    if (!v) continue;
    if (k < 6) atomicMax((unsigned*)box + i, (unsigned)v);
    else atomicAdd(box + i, v);
  }
}

template <typename TP, typename TG>
__global__ void __launch_bounds__(SF_T) k_neighbour_codes(const TP* __restrict__ pred, const TG* __restrict__ gt, int D, int H, int W,
                                                          const cbim_surface_desc* __restrict__ desc, uint8_t* __restrict__ codes,
                                                          int64_t vtot) {
  const cbim_surface_desc d = desc[blockIdx.y];
  const int64_t V = (int64_t)d.nz * d.ny * d.nx;
  for (int64_t i = (int64_t)blockIdx.x * SF_T + threadIdx.x; i < V; i += (int64_t)gridDim.x * SF_T) {
    const int x = d.x0 + (int)(i % d.nx), y = d.y0 + (int)((i / d.nx) % d.ny), z = d.z0 + (int)(i / ((int64_t)d.nx * d.ny));
    int lab[8];
    load8(gt, D, H, W, z, y, x, lab);
    codes[d.off + i] = (uint8_t)code_of(lab, d.cls);
    load8(pred, D, H, W, z, y, x, lab);
    codes[vtot + d.off + i] = (uint8_t)code_of(lab, d.cls);
  }
}

// one wave per x line: surface flags of the line in LDS, every point walks outwards to the nearest flag
__global__ void __launch_bounds__(64) k_edt_x(const cbim_surface_desc* __restrict__ desc, const uint8_t* __restrict__ codes,
                                              int16_t* __restrict__ dx, int64_t vtot) {
  CBIM_DYN_SMEM(flag);
  const cbim_surface_desc d = desc[blockIdx.y];
  const int m = blockIdx.z, nx = d.nx, lines = d.nz * d.ny;
  const uint8_t* cm = codes + (size_t)m * vtot + d.off;
  int16_t* out = dx + (size_t)m * vtot + d.off;
  for (int line = blockIdx.x; line < lines; line += gridDim.x) {
    __syncthreads();
    for (int x = threadIdx.x; x < nx; x += 64) flag[x] = is_surface(cm[(size_t)line * nx + x]) ? 1 : 0;
    __syncthreads();
    for (int x = threadIdx.x; x < nx; x += 64) {
      int res = SF_NONE16;
      for (int r = 0; r < nx; ++r) {
        const bool lo = x - r >= 0, hi = x + r < nx;
        if ((lo && flag[x - r]) || (hi && flag[x + r])) { res = r; break; }
        if (!lo && !hi) break;
      }
      out[(size_t)line * nx + x] = (int16_t)res;
    }
  }
}

// PASS 2: lines along y (stride nx) for every z; src int16 |dx|, dst int32 (|dy| << 16 | |dx|), -1 = no surface point yet.
// PASS 3: lines along z (stride ny*nx) for every y; src that int32; outputs only where the other mask has a surface point.
template <int PASS>
__global__ void __launch_bounds__(SF_T) k_edt_minplus(const cbim_surface_desc* __restrict__ desc, const void* __restrict__ src_,
                                                      int32_t* __restrict__ dst, const uint8_t* __restrict__ codes, int64_t vtot,
                                                      double s0, double s1, double s2, double* __restrict__ out_dist,
                                                      uint8_t* __restrict__ out_code, int64_t out_entries, int* __restrict__ cursor) {
  __shared__ double g[MP_JT][MP_TX];
  __shared__ int s_cnt, s_base;
  const cbim_surface_desc d = desc[blockIdx.y];
  const int m = blockIdx.z, nx = d.nx;
  const int n = PASS == 2 ? d.ny : d.nz, no = PASS == 2 ? d.nz : d.ny;
  const int64_t ls = PASS == 2 ? (int64_t)nx : (int64_t)d.ny * nx, os = PASS == 2 ? (int64_t)d.ny * nx : (int64_t)nx;
  const double sl = PASS == 2 ? s1 : s0;
  const int16_t* src16 = (const int16_t*)src_ + (size_t)m * vtot + d.off;
  const int32_t* src32 = (const int32_t*)src_ + (size_t)m * vtot + d.off;
  const uint8_t* code_other = codes + (size_t)(1 - m) * vtot + d.off;
  const int tx = threadIdx.x & (MP_TX - 1), ty = threadIdx.x >> 5;
  const int xt = (nx + MP_TX - 1) / MP_TX, tiles = no * xt;
  const double inf = INFINITY;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int o = t / xt, col0 = (t % xt) * MP_TX, col = col0 + tx;
    const int64_t base = (int64_t)o * os;
    for (int i0 = 0; i0 < n; i0 += MP_IC) {
      double best[MP_R];
      int arg[MP_R];
      bool need[MP_R];
      bool any = false;
#pragma unroll
      for (int r = 0; r < MP_R; ++r) {
        const int i = i0 + ty + MP_TY * r;
        best[r] = inf;
        arg[r] = -1;
        need[r] = col < nx && i < n;
        if (PASS == 3 && need[r]) need[r] = is_surface(code_other[base + (int64_t)i * ls + col]);
        any = any || need[r];
      }
      for (int j0 = 0; j0 < n; j0 += MP_JT) {
        __syncthreads();
        for (int e = threadIdx.x; e < MP_JT * MP_TX; e += SF_T) {
          const int jj = e >> 5, cx = e & (MP_TX - 1), j = j0 + jj, c = col0 + cx;
          double v = inf;
          if (j < n && c < nx) {
            if (PASS == 2) {
              const int q = src16[base + (int64_t)j * ls + c];
              if (q != SF_NONE16) { const double a = (double)q * s2; v = a * a; }
            } else {
              const int p = src32[base + (int64_t)j * ls + c];
              if (p >= 0) { const double a = (double)(p >> 16) * s1, b = (double)(p & 0xffff) * s2; v = a * a + b * b; }
            }
          }
          g[jj][cx] = v;
        }
        __syncthreads();
        if (any) {
          const int jn = n - j0 < MP_JT ? n - j0 : MP_JT;
          for (int jj = 0; jj < jn; ++jj) {
            const double gj = g[jj][tx];
#pragma unroll
            for (int r = 0; r < MP_R; ++r) {
              const double dd = (double)(i0 + ty + MP_TY * r - (j0 + jj)) * sl;
              const double c = dd * dd + gj;
              if (c < best[r]) { best[r] = c; arg[r] = j0 + jj; }
            }
          }
        }
      }
      if (PASS == 2) {
#pragma unroll
        for (int r = 0; r < MP_R; ++r) {
          const int i = i0 + ty + MP_TY * r;
          if (!need[r]) continue;
          int p = -1;
          if (arg[r] >= 0) p = ((i > arg[r] ? i - arg[r] : arg[r] - i) << 16) | (int)src16[base + (int64_t)arg[r] * ls + col];
          dst[(size_t)m * vtot + d.off + base + (int64_t)i * ls + col] = p;
        }
      } else {
        // append (distance to mask m's surface, own code) to the list of the other mask: slots from an LDS counter, one
        // global atomic per workgroup
        const int A = 1 - m;
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        int mine = 0;
#pragma unroll
        for (int r = 0; r < MP_R; ++r) mine += need[r] ? 1 : 0;
        int slot = mine ? atomicAdd(&s_cnt, mine) : 0;
        __syncthreads();
        if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(cursor + blockIdx.y * 2 + A, s_cnt) : 0;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < MP_R; ++r) {
          const int i = i0 + ty + MP_TY * r;
          if (!need[r]) continue;
          double dist = inf;
          if (arg[r] >= 0) {
            const int p = src32[base + (int64_t)arg[r] * ls + col];
            const double t0 = (double)(i > arg[r] ? i - arg[r] : arg[r] - i) * s0, t1 = (double)(p >> 16) * s1,
                         t2 = (double)(p & 0xffff) * s2;
            dist = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
          }
          const int64_t k = (int64_t)s_base + slot;
          ++slot;
          if (k < d.list_cap[A] && d.list_off[A] + k < out_entries) {     // never past the list the scan sized
            out_dist[d.list_off[A] + k] = dist;
            out_code[d.list_off[A] + k] = code_other[base + (int64_t)i * ls + col];
          }
        }
      }
    }
  }
}

static inline int sf_grid(int64_t items, int per_block, int cap) {
  int64_t b = (items + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace cbim

using namespace cbim;

#define SF_DISPATCH(KERNEL, grid, block, sh, st, ...)                                                                        \
  do {                                                                                                                       \
    if (pred_bytes == 8 && gt_bytes == 8)                                                                                    \
      CBIM_LAUNCH((KERNEL<int64_t, int64_t>), grid, block, sh, st, (const int64_t*)pred, (const int64_t*)gt, __VA_ARGS__);   \
    else if (pred_bytes == 8)                                                                                                \
      CBIM_LAUNCH((KERNEL<int64_t, int8_t>), grid, block, sh, st, (const int64_t*)pred, (const int8_t*)gt, __VA_ARGS__);     \
    else if (gt_bytes == 8)                                                                                                  \
      CBIM_LAUNCH((KERNEL<int8_t, int64_t>), grid, block, sh, st, (const int8_t*)pred, (const int64_t*)gt, __VA_ARGS__);     \
    else                                                                                                                     \
      CBIM_LAUNCH((KERNEL<int8_t, int8_t>), grid, block, sh, st, (const int8_t*)pred, (const int8_t*)gt, __VA_ARGS__);       \
  } while (0)

static int sf_check_volumes(const void* pred, int pred_bytes, const void* gt, int gt_bytes, int D, int H, int W) {
  CBIM_CHECK(pred && gt && D >= 1 && H >= 1 && W >= 1, CBIM_EINVAL, "surface: bad arguments");
  CBIM_CHECK(D < SF_NONE16 - 1 && H < SF_NONE16 - 1 && W < SF_NONE16 - 1, CBIM_EUNSUPPORTED,
             "surface: volume [%d,%d,%d] exceeds the 16-bit offset range", D, H, W);
  CBIM_CHECK((pred_bytes == 1 || pred_bytes == 8) && (gt_bytes == 1 || gt_bytes == 8), CBIM_EUNSUPPORTED,
             "surface: labels must be int8 or int64");
  return CBIM_OK;
}

extern "C" int cbim_surface_scan(const void* pred, int pred_bytes, const void* gt, int gt_bytes, int D, int H, int W, int C,
                                 int32_t* box, void* stream) {
  if (int e = sf_check_volumes(pred, pred_bytes, gt, gt_bytes, D, H, W)) return e;
  CBIM_CHECK(box && C >= 1 && C <= 1024, CBIM_EINVAL, "surface_scan: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  CBIM_LAUNCH(k_surface_zero, dim3(sf_grid(C * 8, SF_T, 64)), dim3(SF_T), 0, st, box, C * 8);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  const int64_t total = (int64_t)(D + 1) * (H + 1) * (W + 1);
  SF_DISPATCH(k_surface_scan, dim3(sf_grid(total, SF_T * 8, 4096)), dim3(SF_T), (size_t)C * 8 * sizeof(int), st, D, H, W, C, box);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH(k_surface_box_decode, dim3(sf_grid(C * 8, SF_T, 64)), dim3(SF_T), 0, st, box, C * 8);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_surface_lists(const void* pred, int pred_bytes, const void* gt, int gt_bytes, int D, int H, int W,
                                  const cbim_surface_desc* desc_host, const cbim_surface_desc* desc_dev, int n, int64_t vtot,
                                  double s0, double s1, double s2, uint8_t* codes, int16_t* dx, int32_t* dyx,
                                  double* out_dist, uint8_t* out_code, int64_t out_entries, int32_t* cursor, void* stream) {
  if (int e = sf_check_volumes(pred, pred_bytes, gt, gt_bytes, D, H, W)) return e;
  CBIM_CHECK(desc_host && desc_dev && n >= 1 && n <= 1024 && vtot >= 1 && codes && dx && dyx && out_dist && out_code && cursor &&
                 out_entries >= 0, CBIM_EINVAL, "surface_lists: bad arguments");
  int64_t max_v = 0;
  int max_lines = 0, max_nx = 0, max_t2 = 0, max_t3 = 0;
  for (int k = 0; k < n; ++k) {
    const cbim_surface_desc& d = desc_host[k];
    CBIM_CHECK(d.nz >= 1 && d.ny >= 1 && d.nx >= 1 && d.z0 >= 0 && d.y0 >= 0 && d.x0 >= 0 && d.z0 + d.nz <= D + 1 &&
                   d.y0 + d.ny <= H + 1 && d.x0 + d.nx <= W + 1, CBIM_EINVAL, "surface_lists: box %d outside the volume", k);
    const int64_t V = (int64_t)d.nz * d.ny * d.nx;
    CBIM_CHECK(d.off >= 0 && d.off + V <= vtot, CBIM_EINVAL, "surface_lists: box %d outside the workspace", k);
    for (int m = 0; m < 2; ++m)
      CBIM_CHECK(d.list_off[m] >= 0 && d.list_cap[m] >= 0 && d.list_off[m] + d.list_cap[m] <= out_entries, CBIM_EINVAL,
                 "surface_lists: list %d/%d outside the output", k, m);
    const int xt = (d.nx + MP_TX - 1) / MP_TX;
    if (V > max_v) max_v = V;
    if (d.nz * d.ny > max_lines) max_lines = d.nz * d.ny;
    if (d.nx > max_nx) max_nx = d.nx;
    if (d.nz * xt > max_t2) max_t2 = d.nz * xt;
    if (d.ny * xt > max_t3) max_t3 = d.ny * xt;
  }
  hipStream_t st = (hipStream_t)stream;
  CBIM_LAUNCH(k_surface_zero, dim3(sf_grid(n * 2, SF_T, 64)), dim3(SF_T), 0, st, cursor, n * 2);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  SF_DISPATCH(k_neighbour_codes, dim3(sf_grid(max_v, SF_T, 2048), n), dim3(SF_T), 0, st, D, H, W, desc_dev, codes, vtot);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH(k_edt_x, dim3(sf_grid(max_lines, 1, 8192), n, 2), dim3(64), (size_t)((max_nx + 15) / 16) * 16, st, desc_dev,
              (const uint8_t*)codes, dx, vtot);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH((k_edt_minplus<2>), dim3(sf_grid(max_t2, 1, 8192), n, 2), dim3(SF_T), 0, st, desc_dev, (const void*)dx, dyx,
              (const uint8_t*)codes, vtot, s0, s1, s2, out_dist, out_code, out_entries, cursor);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  CBIM_LAUNCH((k_edt_minplus<3>), dim3(sf_grid(max_t3, 1, 8192), n, 2), dim3(SF_T), 0, st, desc_dev, (const void*)dyx, (int32_t*)nullptr,
              (const uint8_t*)codes, vtot, s0, s1, s2, out_dist, out_code, out_entries, cursor);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

CBIM_DEFINE_WARM(surface)
