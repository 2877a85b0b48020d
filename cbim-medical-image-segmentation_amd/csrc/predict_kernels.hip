// predict_kernels.hip — the steps of volume prediction below the network (the reference's prediction.py:141-199 and
// dataset_conversion/utils.py:7-33, which run them on the CPU with numpy and SimpleITK):
//
//   k_os_hist / k_os_pick   exact order statistics of a float32 array by radix select: four passes of 8 bits over the
//                           order-preserving integer image of the float bits, one 256-bin histogram per requested rank and
//                           pass (LDS atomics, equal digits of a thread's consecutive elements merged into one atomic), a
//                           one-wave kernel narrows every rank's prefix between the passes — no sort, no host round trip
//   k_bspline_lines         cubic B-spline prefilter along D or H: one thread per line, neighbouring threads on neighbouring
//                           x, so every step of the recursion is a coalesced row access
//   k_bspline_rows          the same recursion along W (contiguous): 256 rows per workgroup, 32-column tiles staged in LDS
//                           (coalesced 128-byte row pieces in and out), each thread walks its own row inside the tile
//   k_resample3d            output voxel -> continuous input index through a 3x4 affine map evaluated in float64, then nearest
//                           (bit copy) / linear (edge-clamped) / cubic (4x4x4 taps on the coefficients, mirrored indices)
//   k_ensemble_finalize     p = prob_sum / counter; total = first ? p : total + p; on the last model the first maximum over
//                           classes as uint8 — one pass per model
//   k_resample_argmax       class probabilities straight to the label map on another grid: per output voxel the taps and weights of
//                           k_resample3d<LINEAR> once, then per class the same trilinear sum (each tap optionally divided by the
//                           window count) and a running first maximum — the K resampled volumes are never written
#include "cbim_common.h"
#include "radix_select.h"   // os_key / os_unkey, os_narrow: shared with topk_kernels.hip

#include <string.h>

namespace cbim {

static constexpr int PR_T = 256;

// ---- order statistics ------------------------------------------------------------------------------------------------------
static constexpr int OS_MAXR = 4;
struct OsRanks { unsigned r[OS_MAXR]; };

// workspace: unsigned hist[4][OS_MAXR][256] | prefix[OS_MAXR] | remaining[OS_MAXR]
__global__ void __launch_bounds__(PR_T) k_os_init(unsigned* __restrict__ ws, OsRanks ranks) {
  for (int i = threadIdx.x; i < 4 * OS_MAXR * 256; i += PR_T) ws[i] = 0u;
  if (threadIdx.x < OS_MAXR) {
    ws[4 * OS_MAXR * 256 + threadIdx.x] = 0u;
    ws[4 * OS_MAXR * 256 + OS_MAXR + threadIdx.x] = ranks.r[threadIdx.x];
  }
}

struct OsRun {
  unsigned bin[OS_MAXR], cnt[OS_MAXR];
};

__device__ __forceinline__ void os_take(float f, int pass, int R, const unsigned* pre, unsigned* sh, OsRun& run) {
  const unsigned key = os_key(f);
  const int shift = 24 - 8 * pass;
  const unsigned digit = (key >> shift) & 255u;
  const unsigned hi = pass == 0 ? 0u : key >> (shift + 8);
#pragma unroll
  for (int j = 0; j < OS_MAXR; ++j) {
    if (j >= R || hi != pre[j]) continue;
    if (run.cnt[j] && run.bin[j] == digit) { ++run.cnt[j]; continue; }
    if (run.cnt[j]) atomicAdd(&sh[j * 256 + run.bin[j]], run.cnt[j]);
    run.bin[j] = digit;
    run.cnt[j] = 1u;
  }
}

// x = head scalar elements | quads 16-byte aligned vectors | tail scalar elements.  In pass 0 all ranks share the (empty) prefix:
// only histogram 0 is filled and k_os_pick reads it for every rank.
__global__ void __launch_bounds__(PR_T) k_os_hist(const float* __restrict__ x, int head, int64_t quads, int tail, int pass, int R,
                                                  unsigned* __restrict__ ws) {
  __shared__ unsigned sh[OS_MAXR * 256];
  for (int i = threadIdx.x; i < OS_MAXR * 256; i += PR_T) sh[i] = 0u;
  unsigned pre[OS_MAXR];
#pragma unroll
  for (int j = 0; j < OS_MAXR; ++j) pre[j] = ws[4 * OS_MAXR * 256 + j];
  const int Rp = pass == 0 ? 1 : R;
  __syncthreads();
  OsRun run;
#pragma unroll
  for (int j = 0; j < OS_MAXR; ++j) { run.bin[j] = 0u; run.cnt[j] = 0u; }
  const f32x4* xv = (const f32x4*)(x + head);
  for (int64_t q = (int64_t)blockIdx.x * PR_T + threadIdx.x; q < quads; q += (int64_t)gridDim.x * PR_T) {
    const f32x4 v = xv[q];
    os_take(v.x, pass, Rp, pre, sh, run);
    os_take(v.y, pass, Rp, pre, sh, run);
    os_take(v.z, pass, Rp, pre, sh, run);
    os_take(v.w, pass, Rp, pre, sh, run);
  }
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < head) os_take(x[threadIdx.x], pass, Rp, pre, sh, run);
    if ((int)threadIdx.x >= 4 && (int)threadIdx.x - 4 < tail) os_take(x[head + 4 * quads + (threadIdx.x - 4)], pass, Rp, pre, sh, run);
  }
#pragma unroll
  for (int j = 0; j < OS_MAXR; ++j)
    if (run.cnt[j]) atomicAdd(&sh[j * 256 + run.bin[j]], run.cnt[j]);
  __syncthreads();
  unsigned* hist = ws + (size_t)pass * OS_MAXR * 256;
  for (int i = threadIdx.x; i < Rp * 256; i += PR_T)
    if (sh[i]) atomicAdd(hist + i, sh[i]);                 // integer atomics: exact, order-independent
}

__global__ void __launch_bounds__(64) k_os_pick(unsigned* __restrict__ ws, int pass, int R, float* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= R) return;
  const unsigned* hist = ws + (size_t)pass * OS_MAXR * 256 + (pass == 0 ? 0 : j * 256);
  unsigned* prefix = ws + 4 * OS_MAXR * 256;
  unsigned* remaining = prefix + OS_MAXR;
  unsigned rem = remaining[j];
  const unsigned d = os_narrow(hist, rem);
  const unsigned p = (prefix[j] << 8) | d;
  prefix[j] = p;
  remaining[j] = rem;
  if (pass == 3) out[j] = os_unkey(p);
}

// ---- cubic B-spline prefilter ------------------------------------------------------------------------------------------------
// One axis of scipy.ndimage.spline_filter1d(order=3, mode='mirror') / ITK's BSplineDecompositionImageFilter in float32: samples
// times the gain 6, c+[0] from the mirrored signal, c+[i] = s[i] + z c+[i-1], c[n-1] = z/(z^2-1) (c+[n-1] + z c+[n-2]),
// c[i] = z (c[i+1] - c+[i]).  The initial sum runs over the whole line up to BS_HZ samples (exact closed form) and over the first
// BS_HZ samples beyond that (|z|^24 = 2e-14, ITK truncates at 1e-10).
static constexpr int BS_HZ = 24;
static constexpr float BS_Z = -0.26794919243112270647f;      // sqrt(3) - 2
static constexpr float BS_GAIN = 6.0f;
static constexpr int BS_TW = 32;                               // columns per LDS tile of the W pass

// s(i): sample i of the line times the gain
template <typename F>
__device__ __forceinline__ float bs_causal_init(int n, F s) {
  const float z = BS_Z;
  if (n > BS_HZ) {
    float zi = z, c0 = s(0);
    for (int i = 1; i < BS_HZ; ++i) { c0 += zi * s(i); zi *= z; }
    return c0;
  }
  float zn1 = 1.f;
  for (int i = 0; i < n - 1; ++i) zn1 *= z;
  float zi = z, c0 = s(0) + zn1 * s(n - 1);
  for (int i = 1; i < n - 1; ++i) { c0 += zi * (s(i) + zn1 * s(n - 1 - i)); zi *= z; }
  return c0 / (1.f - zn1 * zn1);
}

__global__ void __launch_bounds__(PR_T) k_bspline_lines(const float* src, float* dst, int n, int64_t inner,
                                                        int64_t lines) {
  const float z = BS_Z;
  for (int64_t l = (int64_t)blockIdx.x * PR_T + threadIdx.x; l < lines; l += (int64_t)gridDim.x * PR_T) {
    const int64_t base = (l / inner) * n * inner + l % inner;
    const float* sp = src + base;
    float* dp = dst + base;
    float c = bs_causal_init(n, [&](int i) { return sp[(int64_t)i * inner] * BS_GAIN; });
    float prev = c;
    dp[0] = c;
    for (int i = 1; i < n; ++i) {
      prev = c;
      c = sp[(int64_t)i * inner] * BS_GAIN + z * c;
      dp[(int64_t)i * inner] = c;
    }
    c = (z / (z * z - 1.f)) * (c + z * prev);
    dp[(int64_t)(n - 1) * inner] = c;
    for (int i = n - 2; i >= 0; --i) {
      c = z * (c - dp[(int64_t)i * inner]);
      dp[(int64_t)i * inner] = c;
    }
  }
}

// (src may be dst in both kernels: a thread reads a sample before it overwrites it, hence no __restrict__)
// rows of n contiguous samples; thread t of the workgroup owns row blockIdx.x * 256 + t.  tile[r][BS_TW + 1]: the odd row pitch
// spreads the 64 rows a wave walks over the LDS banks.
__global__ void __launch_bounds__(PR_T) k_bspline_rows(const float* src, float* dst, int n, int64_t rows) {
  __shared__ float tile[PR_T][BS_TW + 1];
  const float z = BS_Z;
  const int64_t row0 = (int64_t)blockIdx.x * PR_T;
  const int nrow = rows - row0 < PR_T ? (int)(rows - row0) : PR_T;
  const bool mine = (int)threadIdx.x < nrow;
  const int nt = (n + BS_TW - 1) / BS_TW;
  float c = 0.f, prev = 0.f;
  for (int t = 0; t < nt; ++t) {                               // causal, tiles left to right
    const int c0 = t * BS_TW, cw = n - c0 < BS_TW ? n - c0 : BS_TW;
    __syncthreads();
    for (int e = threadIdx.x; e < PR_T * BS_TW; e += PR_T) {
      const int r = e / BS_TW, cc = e % BS_TW;
      if (r < nrow && cc < cw) tile[r][cc] = src[(row0 + r) * n + c0 + cc] * BS_GAIN;
    }
    __syncthreads();
    if (mine) {
      float* tr = tile[threadIdx.x];
      int i = 0;
      if (t == 0) {                                            // BS_HZ <= BS_TW: the initial sum lies inside the first tile
        c = bs_causal_init(n, [&](int k) { return tr[k]; });
        prev = c;
        tr[0] = c;
        i = 1;
      }
      for (; i < cw; ++i) {
        prev = c;
        c = tr[i] + z * c;
        tr[i] = c;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PR_T * BS_TW; e += PR_T) {
      const int r = e / BS_TW, cc = e % BS_TW;
      if (r < nrow && cc < cw) dst[(row0 + r) * n + c0 + cc] = tile[r][cc];
    }
  }
  c = (z / (z * z - 1.f)) * (c + z * prev);                    // c+[n-1], c+[n-2] are still in registers
  for (int t = nt - 1; t >= 0; --t) {                          // anti-causal, tiles right to left
    const int c0 = t * BS_TW, cw = n - c0 < BS_TW ? n - c0 : BS_TW;
    __syncthreads();
    for (int e = threadIdx.x; e < PR_T * BS_TW; e += PR_T) {
      const int r = e / BS_TW, cc = e % BS_TW;
      if (r < nrow && cc < cw) tile[r][cc] = dst[(row0 + r) * n + c0 + cc];
    }
    __syncthreads();
    if (mine) {
      float* tr = tile[threadIdx.x];
      int i = cw - 1;
      if (t == nt - 1) { tr[i] = c; --i; }
      for (; i >= 0; --i) {
        c = z * (c - tr[i]);
        tr[i] = c;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PR_T * BS_TW; e += PR_T) {
      const int r = e / BS_TW, cc = e % BS_TW;
      if (r < nrow && cc < cw) dst[(row0 + r) * n + c0 + cc] = tile[r][cc];
    }
  }
}

// ---- resampling ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rs_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
__device__ __forceinline__ int rs_mirror(int i, int n) {       // mirror on whole samples, period 2n - 2 (n >= 2)
  const int p = 2 * n - 2;
  int m = i % p;
  if (m < 0) m += p;
  return m >= n ? p - m : m;
}
// cubic B-spline weights of the taps floor(c) - 1 .. floor(c) + 2 at fraction w (the form of ITK's BSplineInterpolateImageFunction)
__device__ __forceinline__ void rs_cubic_w(float w, float o[4]) {
  o[3] = (1.f / 6.f) * w * w * w;
  o[0] = (1.f / 6.f) + 0.5f * w * (w - 1.f) - o[3];
  o[2] = w + o[0] - 2.f * o[3];
  o[1] = 1.f - o[0] - o[2] - o[3];
}

template <int MODE, typename T>
__global__ void __launch_bounds__(PR_T) k_resample3d(const T* __restrict__ src, T* __restrict__ dst, int Di, int Hi, int Wi, int Do,
                                                     int Ho, int Wo, cbim_index_map map, T dflt) {
  const int64_t So = (int64_t)Do * Ho * Wo, Si = (int64_t)Di * Hi * Wi;
  const T* sp = src + (size_t)blockIdx.y * Si;
  T* dp = dst + (size_t)blockIdx.y * So;
  const double* m = map.m;
  for (int64_t o = (int64_t)blockIdx.x * PR_T + threadIdx.x; o < So; o += (int64_t)gridDim.x * PR_T) {
    const int i = (int)(o % Wo), j = (int)((o / Wo) % Ho), k = (int)(o / ((int64_t)Wo * Ho));
    const double cz = ((m[0] * k + m[1] * j) + m[2] * i) + m[3];
    const double cy = ((m[4] * k + m[5] * j) + m[6] * i) + m[7];
    const double cx = ((m[8] * k + m[9] * j) + m[10] * i) + m[11];
    const bool in = cz >= -0.5 && cz < Di - 0.5 && cy >= -0.5 && cy < Hi - 0.5 && cx >= -0.5 && cx < Wi - 0.5;
    if (!in) { dp[o] = dflt; continue; }
    if constexpr (MODE == CBIM_RESAMPLE_NEAREST) {
      const int z = rs_clamp((int)floor(cz + 0.5), Di), y = rs_clamp((int)floor(cy + 0.5), Hi), x = rs_clamp((int)floor(cx + 0.5), Wi);
      dp[o] = sp[((size_t)z * Hi + y) * Wi + x];
    } else {
      const double fz = floor(cz), fy = floor(cy), fx = floor(cx);
      const int bz = (int)fz, by = (int)fy, bx = (int)fx;
      const float tz = (float)(cz - fz), ty = (float)(cy - fy), tx = (float)(cx - fx);
      constexpr int NT = MODE == CBIM_RESAMPLE_LINEAR ? 2 : 4;
      float wz[NT], wy[NT], wx[NT];
      int iz[NT], iy[NT], ix[NT];
      if constexpr (MODE == CBIM_RESAMPLE_LINEAR) {
        wz[0] = 1.f - tz; wz[1] = tz; wy[0] = 1.f - ty; wy[1] = ty; wx[0] = 1.f - tx; wx[1] = tx;
#pragma unroll
        for (int a = 0; a < NT; ++a) { iz[a] = rs_clamp(bz + a, Di); iy[a] = rs_clamp(by + a, Hi); ix[a] = rs_clamp(bx + a, Wi); }
      } else {
        rs_cubic_w(tz, wz); rs_cubic_w(ty, wy); rs_cubic_w(tx, wx);
#pragma unroll
        for (int a = 0; a < NT; ++a) { iz[a] = rs_mirror(bz - 1 + a, Di); iy[a] = rs_mirror(by - 1 + a, Hi); ix[a] = rs_mirror(bx - 1 + a, Wi); }
      }
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        float plane = 0.f;
#pragma unroll
        for (int b = 0; b < NT; ++b) {
          const T* rp = sp + ((size_t)iz[a] * Hi + iy[b]) * Wi;
          float row = 0.f;
#pragma unroll
          for (int c = 0; c < NT; ++c) row += wx[c] * (float)rp[ix[c]];
          plane += wy[b] * row;
        }
        acc += wz[a] * plane;
      }
      dp[o] = (T)acc;
    }
  }
}

// ---- ensemble tail ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PR_T) k_ensemble_finalize(const float* __restrict__ prob_sum, const float* __restrict__ counter,
                                                            float* __restrict__ total, uint8_t* __restrict__ labels, int K, int64_t S,
                                                            int first, int last) {
  for (int64_t v = (int64_t)blockIdx.x * PR_T + threadIdx.x; v < S; v += (int64_t)gridDim.x * PR_T) {
    const float c = counter ? counter[v] : 1.f;
    float best = -INFINITY;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      const size_t e = (size_t)k * S + v;
      float p = prob_sum[e] / c;
      if (!first) p = total[e] + p;
      if (total) total[e] = p;
      if (p > best) { best = p; arg = k; }            // first maximum, like torch.max
    }
    if (last) labels[v] = (uint8_t)arg;
  }
}

// ---- probabilities -> label map on another grid ------------------------------------------------------------------------------------
// What resample3d(linear) over the K channels of prob / counter followed by the first maximum gives, with no [K][Do][Ho][Wo]
// volume in between.  prob and counter point at the first sample of the crop box; sz, sy are the BUFFER's plane and row pitch, Sb
// its channel pitch; Dc, Hc, Wc the box: inside test and clamps see only the box, like resample3d on the sliced-out copy.
// A workgroup owns a box of 64 x 2 x 2 outputs (a wave = 64 neighbours along x): under up-sampling its outputs share source rows
// and planes, so per class the box touches a few hundred bytes that stay in the L1 from the first tap to the last, and the
// channel loop walks K such footprints one channel pitch apart.  Tiles are dealt so that neighbouring ones share an XCD's L2.
static constexpr int RA_TX = 64, RA_TY = 2, RA_TZ = 2;
static_assert(RA_TX * RA_TY * RA_TZ == PR_T, "one output voxel per thread");

template <bool COUNTER>
__global__ void __launch_bounds__(PR_T) k_resample_argmax(const float* __restrict__ prob, const float* __restrict__ counter,
                                                          uint8_t* __restrict__ labels, int K, int64_t Sb, int64_t sz, int64_t sy,
                                                          int Dc, int Hc, int Wc, int Do, int Ho, int Wo, int ntx, int nty,
                                                          int64_t tiles, cbim_index_map map) {
  const double* m = map.m;
  const int lx = threadIdx.x % RA_TX, ly = (threadIdx.x / RA_TX) % RA_TY, lz = threadIdx.x / (RA_TX * RA_TY);
  for (int64_t t = xcd_remap(blockIdx.x, gridDim.x); t < tiles; t += gridDim.x) {
    const int i = (int)(t % ntx) * RA_TX + lx, j = (int)((t / ntx) % nty) * RA_TY + ly, k = (int)(t / ((int64_t)ntx * nty)) * RA_TZ + lz;
    if (i >= Wo || j >= Ho || k >= Do) continue;
    uint8_t* out = labels + ((int64_t)k * Ho + j) * Wo + i;
    const double cz = ((m[0] * k + m[1] * j) + m[2] * i) + m[3];
    const double cy = ((m[4] * k + m[5] * j) + m[6] * i) + m[7];
    const double cx = ((m[8] * k + m[9] * j) + m[10] * i) + m[11];
    const bool in = cz >= -0.5 && cz < Dc - 0.5 && cy >= -0.5 && cy < Hc - 0.5 && cx >= -0.5 && cx < Wc - 0.5;
    if (!in) { *out = 0; continue; }
    const double fz = floor(cz), fy = floor(cy), fx = floor(cx);
    const int bz = (int)fz, by = (int)fy, bx = (int)fx;
    const float tz = (float)(cz - fz), ty = (float)(cy - fy), tx = (float)(cx - fx);
    const float wz[2] = {1.f - tz, tz}, wy[2] = {1.f - ty, ty}, wx[2] = {1.f - tx, tx};
    const int ix[2] = {rs_clamp(bx, Wc), rs_clamp(bx + 1, Wc)};
    int64_t ro[2][2];                                            // row starts inside one channel, shared by all K classes
    float cv[2][2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        ro[a][b] = (int64_t)rs_clamp(bz + a, Dc) * sz + (int64_t)rs_clamp(by + b, Hc) * sy;
        if constexpr (COUNTER) { cv[a][b][0] = counter[ro[a][b] + ix[0]]; cv[a][b][1] = counter[ro[a][b] + ix[1]]; }
      }
    float best = -INFINITY;
    int arg = 0;
    const float* pk = prob;
#pragma unroll 2
    for (int c = 0; c < K; ++c, pk += Sb) {
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        float plane = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float* rp = pk + ro[a][b];
          float row = 0.f;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            float v = rp[ix[e]];
            if constexpr (COUNTER) v = v / cv[a][b][e];          // the division of k_ensemble_finalize, per tap
            row += wx[e] * v;
          }
          plane += wy[b] * row;
        }
        acc += wz[a] * plane;
      }
      if (acc > best) { best = acc; arg = c; }                   // first maximum
    }
    *out = (uint8_t)arg;
  }
}

static inline int pr_grid(int64_t items, int per_block, int cap) {
  int64_t b = (items + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace cbim

using namespace cbim;

#define PR_LAUNCHED() do { if (CBIM_LAST_LAUNCH() != hipSuccess) { cbim_set_error("predict: kernel launch failed"); return CBIM_ELAUNCH; } } while (0)

extern "C" size_t cbim_order_stats_workspace(void) { return (size_t)(4 * OS_MAXR * 256 + 2 * OS_MAXR) * sizeof(unsigned); }

extern "C" int cbim_order_stats_f32(const float* x, int64_t n, const int64_t* ranks, int n_ranks, float* out, void* workspace,
                                    size_t ws_bytes, void* stream) {
  CBIM_CHECK(x && ranks && out && workspace && n >= 1 && n <= ((int64_t)1 << 31), CBIM_EINVAL, "order_stats: bad arguments");
  CBIM_CHECK(n_ranks >= 1 && n_ranks <= OS_MAXR, CBIM_EUNSUPPORTED, "order_stats: 1..%d ranks per call", OS_MAXR);
  CBIM_CHECK(ws_bytes >= cbim_order_stats_workspace(), CBIM_EWORKSPACE, "order_stats: workspace too small");
  CBIM_CHECK(((uintptr_t)x & 3) == 0, CBIM_EINVAL, "order_stats: x is not 4-byte aligned");
  OsRanks rk;
  for (int j = 0; j < OS_MAXR; ++j) {
    const int64_t r = j < n_ranks ? ranks[j] : 0;
    CBIM_CHECK(r >= 0 && r < n, CBIM_EINVAL, "order_stats: rank %lld outside [0, %lld)", (long long)r, (long long)n);
    rk.r[j] = (unsigned)r;
  }
  int head = (int)(((16 - ((uintptr_t)x & 15)) & 15) / 4);
  if (head > n) head = (int)n;
  const int64_t quads = (n - head) / 4;
  const int tail = (int)(n - head - 4 * quads);
  hipStream_t st = (hipStream_t)stream;
  unsigned* ws = (unsigned*)workspace;
  CBIM_LAUNCH(k_os_init, dim3(1), dim3(PR_T), 0, st, ws, rk);
  PR_LAUNCHED();
  for (int pass = 0; pass < 4; ++pass) {
    CBIM_LAUNCH(k_os_hist, dim3(pr_grid(quads, PR_T * 8, 2048)), dim3(PR_T), 0, st, x, head, quads, tail, pass, n_ranks, ws);
    PR_LAUNCHED();
    CBIM_LAUNCH(k_os_pick, dim3(1), dim3(64), 0, st, ws, pass, n_ranks, out);
    PR_LAUNCHED();
  }
  return CBIM_OK;
}

extern "C" int cbim_bspline3_prefilter(const float* src, float* coef, int C, int D, int H, int W, void* stream) {
  CBIM_CHECK(src && coef && C >= 1 && D >= 1 && H >= 1 && W >= 1, CBIM_EINVAL, "bspline3_prefilter: bad arguments");
  CBIM_CHECK(D >= 2 && H >= 2 && W >= 2, CBIM_EUNSUPPORTED, "bspline3_prefilter: every axis of [%d,%d,%d] must hold 2 samples", D, H, W);
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  CBIM_LAUNCH(k_bspline_lines, dim3(pr_grid((int64_t)C * HW, PR_T, 65535)), dim3(PR_T), 0, st, src, coef, D, HW, (int64_t)C * HW);
  PR_LAUNCHED();
  CBIM_LAUNCH(k_bspline_lines, dim3(pr_grid((int64_t)C * D * W, PR_T, 65535)), dim3(PR_T), 0, st, (const float*)coef, coef, H, (int64_t)W,
              (int64_t)C * D * W);
  PR_LAUNCHED();
  const int64_t rows = (int64_t)C * D * H;
  CBIM_CHECK((rows + PR_T - 1) / PR_T <= 0x7fffffff, CBIM_EUNSUPPORTED, "bspline3_prefilter: too many rows");
  CBIM_LAUNCH(k_bspline_rows, dim3((unsigned)((rows + PR_T - 1) / PR_T)), dim3(PR_T), 0, st, (const float*)coef, coef, W, rows);
  PR_LAUNCHED();
  return CBIM_OK;
}

template <int MODE, typename T>
static int rs_launch(const void* src, void* dst, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo, const cbim_index_map& map,
                     T dflt, hipStream_t st) {
  CBIM_LAUNCH((k_resample3d<MODE, T>), dim3(pr_grid((int64_t)Do * Ho * Wo, PR_T, 1 << 20), C), dim3(PR_T), 0, st, (const T*)src, (T*)dst,
              Di, Hi, Wi, Do, Ho, Wo, map, dflt);
  PR_LAUNCHED();
  return CBIM_OK;
}

extern "C" int cbim_resample3d(int mode, const void* src, void* dst, int elem_bytes, int C, int Di, int Hi, int Wi, int Do, int Ho,
                               int Wo, cbim_index_map map, uint32_t default_bits, void* stream) {
  CBIM_CHECK(src && dst && src != dst && C >= 1 && C <= 65535 && Di >= 1 && Hi >= 1 && Wi >= 1 && Do >= 1 && Ho >= 1 && Wo >= 1,
             CBIM_EINVAL, "resample3d: bad arguments");
  CBIM_CHECK(mode == CBIM_RESAMPLE_NEAREST || mode == CBIM_RESAMPLE_LINEAR || mode == CBIM_RESAMPLE_CUBIC, CBIM_EINVAL,
             "resample3d: unknown mode %d", mode);
  for (int a = 0; a < 12; ++a) CBIM_CHECK(map.m[a] == map.m[a] && fabs(map.m[a]) < 1e15, CBIM_EINVAL, "resample3d: index map entry %d is not finite", a);
  hipStream_t st = (hipStream_t)stream;
  if (mode == CBIM_RESAMPLE_NEAREST) {
    CBIM_CHECK(elem_bytes == 1 || elem_bytes == 4, CBIM_EUNSUPPORTED, "resample3d: nearest copies 1-byte or 4-byte elements");
    if (elem_bytes == 1) return rs_launch<CBIM_RESAMPLE_NEAREST, uint8_t>(src, dst, C, Di, Hi, Wi, Do, Ho, Wo, map, (uint8_t)default_bits, st);
    return rs_launch<CBIM_RESAMPLE_NEAREST, uint32_t>(src, dst, C, Di, Hi, Wi, Do, Ho, Wo, map, default_bits, st);
  }
  CBIM_CHECK(elem_bytes == 4, CBIM_EUNSUPPORTED, "resample3d: linear and cubic work on float32");
  CBIM_CHECK(mode != CBIM_RESAMPLE_CUBIC || (Di >= 2 && Hi >= 2 && Wi >= 2), CBIM_EUNSUPPORTED,
             "resample3d: cubic needs 2 samples on every axis of [%d,%d,%d]", Di, Hi, Wi);
  float dflt;
  memcpy(&dflt, &default_bits, 4);
  if (mode == CBIM_RESAMPLE_LINEAR) return rs_launch<CBIM_RESAMPLE_LINEAR, float>(src, dst, C, Di, Hi, Wi, Do, Ho, Wo, map, dflt, st);
  return rs_launch<CBIM_RESAMPLE_CUBIC, float>(src, dst, C, Di, Hi, Wi, Do, Ho, Wo, map, dflt, st);
}

extern "C" int cbim_ensemble_finalize(const float* prob_sum, const float* counter, float* total, uint8_t* labels, int K, int64_t S,
                                      int first, int last, void* stream) {
  CBIM_CHECK(prob_sum && K >= 1 && K <= 256 && S >= 1, CBIM_EINVAL, "ensemble_finalize: bad arguments");
  CBIM_CHECK(total || (first && last), CBIM_EINVAL, "ensemble_finalize: only a single-model ensemble runs without a total buffer");
  CBIM_CHECK(!last || labels, CBIM_EINVAL, "ensemble_finalize: the last model needs the label output");
  CBIM_CHECK(total != prob_sum, CBIM_EINVAL, "ensemble_finalize: total must not alias prob_sum");
  CBIM_LAUNCH(k_ensemble_finalize, dim3(pr_grid(S, PR_T, 1 << 16)), dim3(PR_T), 0, (hipStream_t)stream, prob_sum, counter, total, labels, K,
              S, first, last);
  PR_LAUNCHED();
  return CBIM_OK;
}

extern "C" int cbim_resample_argmax(const float* prob, const float* counter, int K, int Db, int Hb, int Wb, const int* crop,
                                    uint8_t* labels, int Do, int Ho, int Wo, cbim_index_map map, void* stream) {
  CBIM_CHECK(prob && crop && labels, CBIM_EINVAL, "resample_argmax: null pointer");
  CBIM_CHECK(K >= 1 && K <= 256, CBIM_EINVAL, "resample_argmax: %d classes, the label is one byte (1..256)", K);
  CBIM_CHECK(Db >= 1 && Hb >= 1 && Wb >= 1 && Do >= 1 && Ho >= 1 && Wo >= 1, CBIM_EINVAL, "resample_argmax: bad extents");
  const int z0 = crop[0], z1 = crop[1], y0 = crop[2], y1 = crop[3], x0 = crop[4], x1 = crop[5];
  CBIM_CHECK(0 <= z0 && z0 < z1 && z1 <= Db && 0 <= y0 && y0 < y1 && y1 <= Hb && 0 <= x0 && x0 < x1 && x1 <= Wb, CBIM_EINVAL,
             "resample_argmax: crop [%d:%d, %d:%d, %d:%d] is empty or outside the buffer [%d, %d, %d]", z0, z1, y0, y1, x0, x1, Db, Hb, Wb);
  for (int a = 0; a < 12; ++a) CBIM_CHECK(map.m[a] == map.m[a] && fabs(map.m[a]) < 1e15, CBIM_EINVAL, "resample_argmax: index map entry %d is not finite", a);
  const int64_t sy = Wb, sz = (int64_t)Hb * Wb, Sb = (int64_t)Db * sz, first = (int64_t)z0 * sz + (int64_t)y0 * sy + x0;
  const int ntx = (Wo + RA_TX - 1) / RA_TX, nty = (Ho + RA_TY - 1) / RA_TY, ntz = (Do + RA_TZ - 1) / RA_TZ;
  const int64_t tiles = (int64_t)ntx * nty * ntz;
  const dim3 grid(pr_grid(tiles, 1, 1 << 22)), block(PR_T);
  hipStream_t st = (hipStream_t)stream;
  if (counter)
    CBIM_LAUNCH(k_resample_argmax<true>, grid, block, 0, st, prob + first, counter + first, labels, K, Sb, sz, sy, z1 - z0, y1 - y0, x1 - x0,
                Do, Ho, Wo, ntx, nty, tiles, map);
  else
    CBIM_LAUNCH(k_resample_argmax<false>, grid, block, 0, st, prob + first, counter, labels, K, Sb, sz, sy, z1 - z0, y1 - y0, x1 - x0, Do,
                Ho, Wo, ntx, nty, tiles, map);
  PR_LAUNCHED();
  return CBIM_OK;
}

CBIM_DEFINE_WARM(predict)
