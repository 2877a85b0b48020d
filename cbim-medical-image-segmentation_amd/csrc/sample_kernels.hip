// sample_kernels.hip — foreground-oversampled patch sampling for label volumes that stay in HBM.
//
// nnU-Net forces a share of its training patches to contain a voxel of a randomly chosen foreground class; with the
// training set resident on the device the "uniformly random voxel of class c" half of that rule would otherwise be a
// torch.nonzero over the whole label volume plus a device-to-host copy per sample.  Here it is an index built once per
// volume and two short launches per sample, with no host round trip:
//   k_class_index : one read of the label volume -> table int32 [K][nchunk], table[c][j] = voxels of class c in chunk j
//                   (a chunk = ICHUNK consecutive voxels in row-major order), and totals int64 [K+1] (totals[K] = labels
//                   outside [0, K): counted, never indexed with).  Integer atomics only: bitwise reproducible.
//   k_pick_voxel  : ONE workgroup: chooses the class from (mask, totals) and the rank r from the two host draws, finds the
//                   chunk that holds the r-th voxel of the class by a prefix scan over row c of the table (the [K][nchunk]
//                   layout makes that row contiguous) and the voxel inside the chunk by an ordered ballot / popcount
//                   prefix.  Reads K totals, nchunk int32 and one chunk of labels.  Latency-bound: four dependent
//                   round trips (totals, table row, owner's re-walk, chunk labels); a multi-launch scan would only add
//                   launch gaps to them.
//   k_crop3d_at   : k_crop3d (augment_kernels.hip) with the window origin computed from a device coordinate.
#include "atomics_compat.h"
#include "gfx950_prims.h"

namespace cbim {

static constexpr int ICHUNK = 4096;             // voxels per index chunk (cbim_class_index_chunk)
static constexpr int INT = 256;                 // index workgroup: 16 consecutive voxels per thread
static constexpr int IPT = ICHUNK / INT;
static constexpr int PNT = 256;                 // the select workgroup: 4 waves (latency-bound: more waves buy nothing)
static constexpr int PWAVES = PNT / 64;
static constexpr int PROUNDS = ICHUNK / PNT;    // 64-voxel ballot rounds per wave: wave w owns voxels [w, w+1) * 64 * PROUNDS
static constexpr int MAXK = 64;
static constexpr int CNT = 256;
static_assert(IPT == 16 && PROUNDS * PNT == ICHUNK && ICHUNK <= 8192, "chunk geometry");

// class slot of voxel i: its label when inside [0, K), else K (the "ignored" slot)
__device__ __forceinline__ int slot_of(int64_t v, int K) { return v >= 0 && v < K ? (int)v : K; }
__device__ __forceinline__ int slot_at(const void* lab, int lab_bytes, int64_t i, int K) {
  return slot_of(lab_bytes == 1 ? (int64_t)((const int8_t*)lab)[i] : ((const int64_t*)lab)[i], K);
}

__global__ void k_zero_totals(unsigned long long* totals, int n) {
  if ((int)threadIdx.x < n) totals[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(INT) k_class_index(const void* __restrict__ lab, int lab_bytes, int64_t S, int K,
                                                     int nchunk, unsigned long long* __restrict__ totals,
                                                     int* __restrict__ table) {
  __shared__ int sh[MAXK + 1];
  const int t = threadIdx.x;
  for (int j = blockIdx.x; j < nchunk; j += gridDim.x) {
    if (t <= K) sh[t] = 0;
    __syncthreads();
    const int64_t v0 = (int64_t)j * ICHUNK + (int64_t)t * IPT;
    int s[IPT];
    int nv = S - v0 >= IPT ? IPT : (S > v0 ? (int)(S - v0) : 0);
    if (lab_bytes == 1) {
      const int8_t* p = (const int8_t*)lab + v0;
      if (nv == IPT && ((size_t)p & 15) == 0) {            // the aligned interior: one 16-byte load
        const u32x4 q = *(const u32x4*)p;
        const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < IPT; ++k) s[k] = slot_of((int64_t)(int8_t)((wd[k >> 2] >> (8 * (k & 3))) & 0xffu), K);
      } else {
#pragma unroll
        for (int k = 0; k < IPT; ++k) s[k] = k < nv ? slot_of((int64_t)p[k], K) : -1;
      }
    } else {
      const int64_t* p = (const int64_t*)lab + v0;
#pragma unroll
      for (int k = 0; k < IPT; ++k) s[k] = k < nv ? slot_of(p[k], K) : -1;
    }
    // neighbouring voxels mostly share a label: one LDS atomic per run of equal slots (integer: exact, order-independent)
    int cur = -1, cnt = 0;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      if (k < nv) {
        if (s[k] == cur) ++cnt;
        else {
          if (cnt) atomicAdd(&sh[cur], cnt);
          cur = s[k]; cnt = 1;
        }
      }
    }
    if (cnt) atomicAdd(&sh[cur], cnt);
    __syncthreads();
    if (t <= K) {
      const int n = sh[t];
      if (t < K) table[(size_t)t * nchunk + j] = n;
      if (n) atomicAdd(totals + t, (unsigned long long)n);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void put4(int* out, int a, int b, int c, int d) { out[0] = a; out[1] = b; out[2] = c; out[3] = d; }

__global__ void __launch_bounds__(PNT) k_pick_voxel(const void* __restrict__ lab, int lab_bytes, int H, int W, int64_t S,
                                                    int K, int nchunk, const long long* __restrict__ totals,
                                                    const int* __restrict__ table, unsigned long long class_mask,
                                                    double u_class, double u_rank, int* __restrict__ out) {
  __shared__ long long s_wave[PWAVES];
  __shared__ long long s_rem;
  __shared__ int s_chunk, s_found;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

  // ---- the class: every wave forms the same ordered list of eligible classes (lane c <-> class c) ------------------------
  const long long tot = lane < K ? totals[lane] : 0;
  const unsigned long long elig = wave_ballot(tot > 0 && ((class_mask >> lane) & 1ull));
  const int n = __builtin_popcountll(elig);
  if (n == 0) {                                              // block-uniform: nothing to pick
    if (t == 0) put4(out, -1, -1, -1, -1);
    return;
  }
  long long pos = (long long)(u_class * (double)n);
  if (pos > n - 1) pos = n - 1;
  unsigned long long m = elig;
  for (long long i = 0; i < pos; ++i) m &= m - 1;            // drop the `pos` lowest eligible classes
  const int c = __builtin_ctzll(m);
  const long long T = __shfl(tot, c, 64);
  long long r = (long long)(u_rank * (double)T);
  if (r > T - 1) r = T - 1;

  // ---- the chunk: thread t owns elements [t seg, (t+1) seg) of row c; block-wide exclusive prefix of the owners' sums -----
  const int* row = table + (size_t)c * nchunk;
  const int seg = (nchunk + PNT - 1) / PNT;
  const int e0 = t * seg < nchunk ? t * seg : nchunk, e1 = e0 + seg < nchunk ? e0 + seg : nchunk;
  long long mine = 0;
  for (int e = e0; e < e1; ++e) mine += row[e];
  const long long inc = wave_scan_incl(mine, lane);
  if (lane == 63) s_wave[wave] = inc;
  if (t == 0) { s_chunk = -1; s_found = 0; }
  __syncthreads();
  long long ex = inc - mine;
  for (int w = 0; w < wave; ++w) ex += s_wave[w];
  if (ex <= r && r < ex + mine) {                            // exactly one thread, unless the index does not belong to totals
    long long run = ex;
    int e = e0;
    for (; e < e1; ++e) {
      const long long v = row[e];
      if (r < run + v) break;
      run += v;
    }
    s_chunk = e;                                             // < e1 <= nchunk: r < ex + mine ends the walk inside the segment
    s_rem = r - run;
  }
  __syncthreads();
  const int j = s_chunk;
  if (j < 0) {                                               // block-uniform
    if (t == 0) put4(out, -1, -1, -1, -1);
    return;
  }

  // ---- the voxel: rem-th voxel of class c inside chunk j, by ordered ballots ----------------------------------------------
  const long long rem = s_rem;
  const int64_t vb = (int64_t)j * ICHUNK + (int64_t)wave * (64 * PROUNDS) + lane;
  int lb[PROUNDS];
#pragma unroll
  for (int k = 0; k < PROUNDS; ++k) {                        // the loads first: one latency for all rounds
    const int64_t v = vb + k * 64;
    lb[k] = v < S ? slot_at(lab, lab_bytes, v, K) : -1;
  }
  unsigned long long msk[PROUNDS];
  int wcnt = 0;
#pragma unroll
  for (int k = 0; k < PROUNDS; ++k) {
    msk[k] = wave_ballot(lb[k] == c);
    wcnt += __builtin_popcountll(msk[k]);
  }
  if (lane == 0) s_wave[wave] = wcnt;                        // every read of the row sums happened before the last barrier
  __syncthreads();
  long long before = 0;
  for (int w = 0; w < wave; ++w) before += s_wave[w];
  if (before <= rem && rem < before + wcnt) {                // wave-uniform: this wave holds the voxel
    int need = (int)(rem - before);
    bool done = false;
#pragma unroll
    for (int k = 0; k < PROUNDS; ++k) {
      const int pc = __builtin_popcountll(msk[k]);
      if (!done && need < pc) {
        if (((msk[k] >> lane) & 1ull) && ballot_rank(msk[k], lane) == need) {
          const int64_t v = vb + k * 64;
          const int64_t hw = (int64_t)H * W;
          put4(out, (int)(v / hw), (int)((v / W) % H), (int)(v % W), c);
          s_found = 1;
        }
        done = true;
      }
      if (!done) need -= pc;
    }
  }
  __syncthreads();
  if (t == 0 && !s_found) put4(out, -1, -1, -1, -1);         // labels changed after the index was built
}

__global__ void __launch_bounds__(CNT) k_crop3d_at(const float* img, const void* lab, float* oimg, void* olab, int C,
                                                   int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                                   const int* __restrict__ coord, int jz, int jy, int jx, int fz, int fy,
                                                   int fx, int lab_bytes) {
  int d0 = fz, h0 = fy, w0 = fx;
  const int cz = coord[0];
  if (cz >= 0) {                                             // 64-bit: a coordinate is data, whatever it holds the origin is clamped
    const int64_t a = (int64_t)cz - jz, b = (int64_t)coord[1] - jy, c = (int64_t)coord[2] - jx;
    d0 = (int)(a < 0 ? 0 : (a > Di - Do ? Di - Do : a));
    h0 = (int)(b < 0 ? 0 : (b > Hi - Ho ? Hi - Ho : b));
    w0 = (int)(c < 0 ? 0 : (c > Wi - Wo ? Wi - Wo : c));
  }
  const int64_t total = (int64_t)Do * Ho * Wo, Sin = (int64_t)Di * Hi * Wi;
  for (int64_t i = (int64_t)blockIdx.x * CNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * CNT) {
    int w = (int)(i % Wo);
    int64_t r = i / Wo;
    int h = (int)(r % Ho), d = (int)(r / Ho);
    int64_t o = ((int64_t)(d0 + d) * Hi + (h0 + h)) * Wi + (w0 + w);
    for (int ch = 0; ch < C; ++ch) oimg[(int64_t)ch * total + i] = img[(int64_t)ch * Sin + o];
    if (lab) {
      if (lab_bytes == 1) ((int8_t*)olab)[i] = ((const int8_t*)lab)[o];
      else ((int64_t*)olab)[i] = ((const int64_t*)lab)[o];
    }
  }
}

static inline int64_t chunks_of(int64_t S) { return (S + ICHUNK - 1) / ICHUNK; }

}  // namespace cbim

using namespace cbim;

static int launch_status(const char* what) {
  hipError_t e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "%s launch: %s", what, hipGetErrorString(e));
  return CBIM_OK;
}

extern "C" int cbim_class_index_chunk(void) { return ICHUNK; }

extern "C" int cbim_class_index(const void* lab, int lab_bytes, int64_t S, int K, int64_t* totals, int32_t* table,
                                void* stream) {
  CBIM_CHECK(lab && totals && table, CBIM_EINVAL, "null argument");
  CBIM_CHECK(lab_bytes == 1 || lab_bytes == 8, CBIM_EUNSUPPORTED, "label must be int8 or int64");
  CBIM_CHECK(K >= 2 && K <= MAXK, CBIM_EINVAL, "class count %d outside [2, %d]", K, MAXK);
  CBIM_CHECK(S > 0 && chunks_of(S) <= (int64_t)1 << 24, CBIM_EINVAL, "volume of %lld voxels unsupported", (long long)S);
  const int nchunk = (int)chunks_of(S);
  hipStream_t st = (hipStream_t)stream;
  CBIM_LAUNCH(k_zero_totals, dim3(1), dim3(128), 0, st, (unsigned long long*)totals, K + 1);
  if (int e = launch_status("class_index (zero)")) return e;
  CBIM_LAUNCH(k_class_index, dim3(nchunk < 2048 ? nchunk : 2048), dim3(INT), 0, st, lab, lab_bytes, S, K, nchunk,
              (unsigned long long*)totals, (int*)table);
  return launch_status("class_index");
}

extern "C" int cbim_pick_voxel(const void* lab, int lab_bytes, int D, int H, int W, int K, const int64_t* totals,
                               const int32_t* table, uint64_t class_mask, double u_class, double u_rank, int32_t* out,
                               void* stream) {
  CBIM_CHECK(lab && totals && table && out, CBIM_EINVAL, "null argument");
  CBIM_CHECK(lab_bytes == 1 || lab_bytes == 8, CBIM_EUNSUPPORTED, "label must be int8 or int64");
  CBIM_CHECK(K >= 2 && K <= MAXK, CBIM_EINVAL, "class count %d outside [2, %d]", K, MAXK);
  CBIM_CHECK(D > 0 && H > 0 && W > 0, CBIM_EINVAL, "bad volume %dx%dx%d", D, H, W);
  CBIM_CHECK(u_class >= 0.0 && u_class < 1.0 && u_rank >= 0.0 && u_rank < 1.0, CBIM_EINVAL,
             "draws (%g, %g) outside [0, 1)", u_class, u_rank);
  const int64_t S = (int64_t)D * H * W;
  CBIM_CHECK(chunks_of(S) <= (int64_t)1 << 24, CBIM_EINVAL, "volume of %lld voxels unsupported", (long long)S);
  CBIM_LAUNCH(k_pick_voxel, dim3(1), dim3(PNT), 0, (hipStream_t)stream, lab, lab_bytes, H, W, S, K, (int)chunks_of(S),
              (const long long*)totals, (const int*)table, (unsigned long long)class_mask, u_class, u_rank, (int*)out);
  return launch_status("pick_voxel");
}

extern "C" int cbim_crop3d_at(const float* img, const void* lab, int lab_bytes, float* out_img, void* out_lab, int C,
                              int Di, int Hi, int Wi, int Do, int Ho, int Wo, const int32_t* coord, int jz, int jy, int jx,
                              int fz, int fy, int fx, void* stream) {
  CBIM_CHECK(img && out_img && coord, CBIM_EINVAL, "null argument");
  CBIM_CHECK(!lab || (out_lab && (lab_bytes == 1 || lab_bytes == 8)), CBIM_EUNSUPPORTED, "label must be int8 or int64");
  CBIM_CHECK(C > 0 && Do > 0 && Ho > 0 && Wo > 0 && Do <= Di && Ho <= Hi && Wo <= Wi, CBIM_EINVAL,
             "crop %dx%dx%d larger than the %dx%dx%d volume", Do, Ho, Wo, Di, Hi, Wi);
  CBIM_CHECK(jz >= 0 && jy >= 0 && jx >= 0, CBIM_EINVAL, "negative offset of the voxel inside the window");
  CBIM_CHECK(fz >= 0 && fy >= 0 && fx >= 0 && fz + Do <= Di && fy + Ho <= Hi && fx + Wo <= Wi, CBIM_EINVAL,
             "fallback window outside the volume");
  int64_t b = ((int64_t)Do * Ho * Wo + CNT - 1) / CNT;
  if (b > 256 * 8) b = 256 * 8;
  CBIM_LAUNCH(k_crop3d_at, dim3((int)b), dim3(CNT), 0, (hipStream_t)stream, img, lab, out_img, out_lab, C, Di, Hi, Wi,
              Do, Ho, Wo, (const int*)coord, jz, jy, jx, fz, fy, fx, lab_bytes);
  return launch_status("crop3d_at");
}

CBIM_DEFINE_WARM(sample)
