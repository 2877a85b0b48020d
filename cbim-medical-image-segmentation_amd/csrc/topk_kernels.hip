// topk_kernels.hip — top-k cross entropy (the mean of the K largest per-voxel weighted CE terms of the batch: online hard-example
// mining, nnU-Net's TopKLoss), optionally fused with the soft Dice loss of loss_kernels.hip, in one pass over the logits.
//
// Composed from torch ops this is cross_entropy(reduction="none") + torch.topk (a sort of N*S values) + the ~10 full-size
// temporaries of the Dice formula.  Here:
//   k_topk_fwd       one read of logits and labels: nll_i = w[y_i] (logsumexp(z_i) - z_i[y_i]) to the workspace (float32 [N*S], 1/C of
//                    the logits' bytes) and, with DICE, the TP / SP / CNT workgroup records of k_dice_ce_fwd statement for statement
//   k_topk_hist/pick the exact threshold tau = the K-th largest nll by radix select over the nll array alone (radix_select.h: four
//                    8-bit passes over the order-preserving key; integer atomics only), with n_gt = #{nll > tau} and n_eq = #{nll = tau}
//   k_topk_sum       per workgroup the fp64 sum of the values above tau, fixed order
//   k_topk_finalize  single workgroup, fp64: topk = (sum_{nll > tau} nll + (K - n_gt) tau) / K — any choice among the values equal to
//                    tau gives this number —, the Dice term and its coefficients (loss_common.h), and the record the backward reads
//   k_topk_bwd       one read of logits, labels and nll, one write: a voxel's CE gradient w[y] (p - onehot) times 1/K above tau,
//                    (K - n_gt) / (n_eq K) at tau (the ties share what is left of K evenly: deterministic), 0 below
// No host synchronisation, no allocation, no float atomics: every result is bitwise reproducible and the calls can be captured.
// A label outside [0, C) is never used as an index: nll = 0, no gradient, no TP / CNT, and it is counted.
#include "loss_common.h"
#include "radix_select.h"

namespace cbim {

static constexpr int TK_SUMS = 1024;   // upper bound of k_topk_sum's grid (one fp64 record per workgroup)

// workspace: nll float[total, padded to 4] | partials float[loss_blocks][3C + 1] | sums double[TK_SUMS] |
//            hist unsigned[4][256] | state unsigned[4] = prefix, rank left, n_gt, keys under the prefix | rec float[4] = tau, 1/K, tie weight
struct TopkWs {
  float* nll;
  float* partials;
  double* sums;
  unsigned* hist;
  unsigned* state;
  float* rec;
  size_t bytes;
};
static inline size_t tk_up16(size_t b) { return (b + 15) & ~(size_t)15; }
static inline TopkWs topk_layout(void* base, int N, int C, int64_t S) {
  const int64_t total = (int64_t)N * S;
  char* p = (char*)base;
  size_t o = 0;
  TopkWs w;
  w.nll = (float*)(p + o);      o += tk_up16((size_t)total * sizeof(float));
  w.partials = (float*)(p + o); o += tk_up16((size_t)loss_blocks(total) * (3 * C + 1) * sizeof(float));
  w.sums = (double*)(p + o);    o += TK_SUMS * sizeof(double);
  w.hist = (unsigned*)(p + o);  o += 4 * 256 * sizeof(unsigned);
  w.state = (unsigned*)(p + o); o += 4 * sizeof(unsigned);
  w.rec = (float*)(p + o);      o += 4 * sizeof(float);
  w.bytes = o;
  return w;
}

// fixed-order fp64 sum over the NT threads of a workgroup (valid in thread 0)
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// partial layout per workgroup: DICE: [3*C + 1] = TP[C], SP[C], CNT[C], #labels outside [0, C);  else [1].
// Workgroup 0 also clears the histograms and sets the select's state: every k_topk_hist launch follows this kernel on the stream.
template <int CT, int V, bool DICE>
__global__ void __launch_bounds__(NT) k_topk_fwd(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                 const float* __restrict__ wgt, int C, int64_t S, int64_t groups,
                                                 float* __restrict__ nll, float* __restrict__ partials,
                                                 unsigned* __restrict__ hist, unsigned rank, unsigned total) {
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < 4 * 256; i += NT) hist[i] = 0u;
    if (threadIdx.x == 0) { hist[1024] = 0u; hist[1025] = rank; hist[1026] = 0u; hist[1027] = total; }
  }
  constexpr int CA = DICE ? CT : 1;
  float tp[CA], sp[CA], cnt[CA];
#pragma unroll
  for (int c = 0; c < CA; ++c) { tp[c] = 0.f; sp[c] = 0.f; cnt[c] = 0.f; }
  float bad = 0.f;
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < groups; g += (int64_t)gridDim.x * NT) {
    const int64_t r = g * V;
    const int64_t n = r / S, v = r % S;
    const float* zp = z + (size_t)n * C * S + v;
    int lab[V];
#pragma unroll
    for (int i = 0; i < V; ++i) lab[i] = (int)y[r + i];
    float l[CT][V];
    float mx[V], zy[V], se[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = -INFINITY; zy[i] = 0.f; se[i] = 0.f; }
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) ldv<V>(zp + (size_t)c * S, l[c]);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
#pragma unroll
        for (int i = 0; i < V; ++i) { mx[i] = fmaxf(mx[i], l[c][i]); if (c == lab[i]) zy[i] = l[c][i]; }
      }
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
#pragma unroll
        for (int i = 0; i < V; ++i) { l[c][i] = __expf(l[c][i] - mx[i]); se[i] += l[c][i]; }
      }
    if constexpr (DICE) {
      float inv[V];
#pragma unroll
      for (int i = 0; i < V; ++i) inv[i] = 1.f / se[i];
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
#pragma unroll
          for (int i = 0; i < V; ++i) {
            float pc = l[c][i] * inv[i];
            sp[c] += pc;
            if (c == lab[i]) { tp[c] += pc; cnt[c] += 1.f; }
          }
        }
    }
    float o[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const bool ok = (unsigned)lab[i] < (unsigned)C;
      float wy = ok ? (wgt ? wgt[lab[i]] : 1.f) : 0.f;
      o[i] = wy * (__logf(se[i]) + mx[i] - zy[i]) + 0.f;   // + 0: no -0, whose key differs from +0's
      bad += ok ? 0.f : 1.f;
    }
    stv<V>(nll + r, o);
  }
  // workgroup reduction (fixed order): wave shuffles then 4 waves through LDS
  constexpr int NR = DICE ? 3 * CT + 1 : 1;
  constexpr int BO = DICE ? 3 * CT : 0;               // where the count sits in a wave's row
  __shared__ float red[4][NR];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if constexpr (DICE) {
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      if (c < C) {
        float a = wave_sum(tp[c]), b = wave_sum(sp[c]), d = wave_sum(cnt[c]);
        if (lane == 0) { red[wave][c] = a; red[wave][CT + c] = b; red[wave][2 * CT + c] = d; }
      }
    }
  }
  {
    float e = wave_sum(bad);
    if (lane == 0) red[wave][BO] = e;
  }
  __syncthreads();
  const int nd = DICE ? 3 * C : 0;
  float* out = partials + (size_t)blockIdx.x * (nd + 1);
  for (int i = threadIdx.x; i < nd + 1; i += NT) {
    int src = i < nd ? (i / C) * CT + (i % C) : BO;
    out[i] = red[0][src] + red[1][src] + red[2][src] + red[3][src];
  }
}

// One 8-bit pass of the select over x = quads 16-byte vectors | tail scalar elements: the digits of the keys under the prefix the
// earlier passes fixed.  A thread merges equal digits of the elements it meets in a row into one LDS atomic (pass 0 sees two or three
// exponent bins for nearly every value: one atomic per thread, not per element); each wave has its own 256 bins.
__device__ __forceinline__ void tk_take(float f, int shift, bool all, unsigned pre, unsigned* sh, unsigned& bin, unsigned& cnt) {
  const unsigned key = os_key(f);
  if (!all && (key >> (shift + 8)) != pre) return;
  const unsigned digit = (key >> shift) & 255u;
  if (cnt && bin == digit) { ++cnt; return; }
  if (cnt) atomicAdd(&sh[bin], cnt);
  bin = digit;
  cnt = 1u;
}

__global__ void __launch_bounds__(NT) k_topk_hist(const float* __restrict__ x, int64_t quads, int tail, int pass,
                                                  unsigned* __restrict__ hist) {
  __shared__ unsigned sh[4 * 256];
  for (int i = threadIdx.x; i < 4 * 256; i += NT) sh[i] = 0u;
  const unsigned pre = hist[1024];
  __syncthreads();
  unsigned* mine = sh + (threadIdx.x >> 6) * 256;
  const int shift = 24 - 8 * pass;
  const bool all = pass == 0;
  unsigned bin = 0u, cnt = 0u;
  const f32x4* xv = (const f32x4*)x;
  for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < quads; q += (int64_t)gridDim.x * NT) {
    const f32x4 v = xv[q];
    tk_take(v.x, shift, all, pre, mine, bin, cnt);
    tk_take(v.y, shift, all, pre, mine, bin, cnt);
    tk_take(v.z, shift, all, pre, mine, bin, cnt);
    tk_take(v.w, shift, all, pre, mine, bin, cnt);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) tk_take(x[4 * quads + threadIdx.x], shift, all, pre, mine, bin, cnt);
  if (cnt) atomicAdd(&mine[bin], cnt);
  __syncthreads();
  unsigned* out = hist + pass * 256;
  for (int i = threadIdx.x; i < 256; i += NT) {
    const unsigned c = (sh[i] + sh[256 + i]) + (sh[512 + i] + sh[768 + i]);
    if (c) atomicAdd(out + i, c);                       // integer atomics: exact, order-independent
  }
}

// Narrow the rank to one digit of this pass's histogram (os_narrow on an LDS copy) and keep count of the keys above: those of the
// bins over the chosen one are larger than the element sought whatever their lower bits.
__global__ void __launch_bounds__(NT) k_topk_pick(unsigned* __restrict__ hist, int pass, float* __restrict__ rec) {
  __shared__ unsigned sh[256];
  sh[threadIdx.x] = hist[pass * 256 + threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned* state = hist + 1024;
  const unsigned before = state[1];
  unsigned rem = before;
  const unsigned d = os_narrow(sh, rem);
  const unsigned c = sh[d];
  const unsigned p = (state[0] << 8) | d;
  state[0] = p;
  state[1] = rem;
  state[2] += state[3] - (before - rem) - c;
  state[3] = c;                                          // after the last pass: the number of values equal to tau
  if (pass == 3) rec[0] = os_unkey(p);
}

__global__ void __launch_bounds__(NT) k_topk_sum(const float* __restrict__ x, int64_t quads, int tail,
                                                 const float* __restrict__ rec, double* __restrict__ sums) {
  __shared__ double sh[NT];
  const float tau = rec[0];
  double acc = 0.0;
  const f32x4* xv = (const f32x4*)x;
  for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < quads; q += (int64_t)gridDim.x * NT) {
    const f32x4 v = xv[q];
    acc += (double)(v.x > tau ? v.x : 0.f);
    acc += (double)(v.y > tau ? v.y : 0.f);
    acc += (double)(v.z > tau ? v.z : 0.f);
    acc += (double)(v.w > tau ? v.w : 0.f);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
    const float f = x[4 * quads + threadIdx.x];
    acc += (double)(f > tau ? f : 0.f);
  }
  const double s = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// single workgroup: out = (top-k + Dice, top-k term, Dice, #bad labels, top-k + Dice as the float32 sum of the two entries).
// DICE: coef as k_dice_ce_finalize leaves it ([2][C] class coefficients, [C] per-class terms at 2C + 1); coef[2C] = 1/K.
template <bool DICE>
__global__ void __launch_bounds__(NT) k_topk_finalize(const float* __restrict__ partials, int nblk, int C,
                                                      const double* __restrict__ sums, int nsum,
                                                      const unsigned* __restrict__ state, double K,
                                                      float* __restrict__ rec, float* __restrict__ out,
                                                      float* __restrict__ coef) {
  __shared__ double tot[3 * CMAX + 3];
  __shared__ double part[4][3 * CMAX + 3];
  __shared__ double dice_term[CMAX];
  __shared__ double sh[NT];
  const int nd = DICE ? 3 * C : 0;
  loss_reduce_partials(partials, nblk, nd + 1, tot, part);
  if constexpr (DICE) {
    if ((int)threadIdx.x < C) {
      int c = threadIdx.x;
      dice_term[c] = dice_class_term(tot[c], tot[C + c], tot[2 * C + c], C, c, coef);
    }
  }
  double acc = 0.0;
  for (int i = threadIdx.x; i < nsum; i += NT) acc += sums[i];
  const double above = block_sum_f64(acc, sh);          // (its barriers also publish dice_term)
  if (threadIdx.x == 0) {
    double dl = 0.0;
    if constexpr (DICE) {
      for (int c = 0; c < C; ++c) dl += dice_term[c];
      dl /= C;
      coef[2 * C] = (float)(1.0 / K);
    }
    const double tau = (double)rec[0], n_gt = (double)state[2], n_eq = (double)state[3];
    const double tk = (above + (K - n_gt) * tau) / K;
    rec[1] = (float)(1.0 / K);
    rec[2] = (float)((K - n_gt) / (n_eq * K));
    const float ftk = (float)tk, fdice = (float)dl;
    out[0] = (float)(tk + dl);
    out[1] = ftk;
    out[2] = fdice;
    out[3] = (float)tot[nd];      // labels outside [0, C)
    out[4] = ftk + fdice;         // the float32 sum of the two entries, as adding them on the host side would give
  }
}

// dlogits = g_topk * d topk/dz [+ g_dice * dDice/dz]   (grad_out = {g_topk, g_dice} on the device)
template <int CT, int V, bool DICE>
__global__ void __launch_bounds__(NT) k_topk_bwd(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                 const float* __restrict__ wgt, const float* __restrict__ coef,
                                                 const float* __restrict__ grad_out, const float* __restrict__ nll,
                                                 const float* __restrict__ rec, float* __restrict__ dz, int C,
                                                 int64_t S, int64_t groups) {
  __shared__ float cf[2 * CMAX];
  if constexpr (DICE) {
    if ((int)threadIdx.x < 2 * C) cf[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
  }
  const float g_tk = grad_out[0], g_dice = DICE ? grad_out[1] : 0.f;
  const float tau = rec[0], w_gt = g_tk * rec[1], w_eq = g_tk * rec[2];
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < groups; g += (int64_t)gridDim.x * NT) {
    const int64_t r = g * V;
    const int64_t n = r / S, v = r % S;
    const float* zp = z + (size_t)n * C * S + v;
    float* dp = dz + (size_t)n * C * S + v;
    int lab[V];
#pragma unroll
    for (int i = 0; i < V; ++i) lab[i] = (int)y[r + i];
    float l[CT][V];
    float mx[V], se[V], dot[V], wy[V], e[V];
    ldv<V>(nll + r, e);
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = -INFINITY; se[i] = 0.f; dot[i] = 0.f; }
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) ldv<V>(zp + (size_t)c * S, l[c]);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
#pragma unroll
        for (int i = 0; i < V; ++i) mx[i] = fmaxf(mx[i], l[c][i]);
      }
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
#pragma unroll
        for (int i = 0; i < V; ++i) { l[c][i] = __expf(l[c][i] - mx[i]); se[i] += l[c][i]; }
      }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      se[i] = 1.f / se[i];
      const bool ok = (unsigned)lab[i] < (unsigned)C;     // see k_topk_fwd: such a voxel only feeds SP
      const float sel = e[i] > tau ? w_gt : (e[i] == tau ? w_eq : 0.f);
      wy[i] = ok ? (wgt ? wgt[lab[i]] : 1.f) * sel : 0.f;
    }
    if constexpr (DICE) {
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          const float gs = cf[C + c], gt = cf[c];
#pragma unroll
          for (int i = 0; i < V; ++i) {
            l[c][i] *= se[i];
            dot[i] += l[c][i] * (gs + (c == lab[i] ? gt : 0.f));   // sum_k p_k G_k
          }
        }
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
#pragma unroll
          for (int i = 0; i < V; ++i) l[c][i] *= se[i];
        }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
        float o[V];
        if constexpr (DICE) {
          const float gs = cf[C + c], gt = cf[c];
#pragma unroll
          for (int i = 0; i < V; ++i) {
            float G = gs + (c == lab[i] ? gt : 0.f);
            float d_dice = l[c][i] * (G - dot[i]);
            o[i] = wy[i] * (l[c][i] - (c == lab[i] ? 1.f : 0.f)) + g_dice * d_dice;
          }
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] = wy[i] * (l[c][i] - (c == lab[i] ? 1.f : 0.f));
        }
        stv<V>(dp + (size_t)c * S, o);
      }
  }
}

template <bool DICE>
static void topk_launch_fwd(int C, int V, int nb, hipStream_t st, const float* logits, const int64_t* labels,
                            const float* weight, int64_t S, int64_t groups, const TopkWs& w, unsigned rank, unsigned total) {
  if (C <= 16) {
    if (V == 4) CBIM_LAUNCH((k_topk_fwd<16, 4, DICE>), dim3(nb), dim3(NT), 0, st, logits, labels, weight, C, S, groups, w.nll, w.partials, w.hist, rank, total);
    else CBIM_LAUNCH((k_topk_fwd<16, 1, DICE>), dim3(nb), dim3(NT), 0, st, logits, labels, weight, C, S, groups, w.nll, w.partials, w.hist, rank, total);
  } else {
    if (V == 2) CBIM_LAUNCH((k_topk_fwd<CMAX, 2, DICE>), dim3(nb), dim3(NT), 0, st, logits, labels, weight, C, S, groups, w.nll, w.partials, w.hist, rank, total);
    else CBIM_LAUNCH((k_topk_fwd<CMAX, 1, DICE>), dim3(nb), dim3(NT), 0, st, logits, labels, weight, C, S, groups, w.nll, w.partials, w.hist, rank, total);
  }
}

template <bool DICE>
static void topk_launch_bwd(int C, int V, dim3 grid, hipStream_t st, const float* logits, const int64_t* labels,
                            const float* weight, const float* coef, const float* grad_out, const TopkWs& w,
                            float* dlogits, int64_t S, int64_t groups) {
  if (C <= 16) {
    if (V == 4) CBIM_LAUNCH((k_topk_bwd<16, 4, DICE>), grid, dim3(NT), 0, st, logits, labels, weight, coef, grad_out, (const float*)w.nll, (const float*)w.rec, dlogits, C, S, groups);
    else CBIM_LAUNCH((k_topk_bwd<16, 1, DICE>), grid, dim3(NT), 0, st, logits, labels, weight, coef, grad_out, (const float*)w.nll, (const float*)w.rec, dlogits, C, S, groups);
  } else {
    if (V == 2) CBIM_LAUNCH((k_topk_bwd<CMAX, 2, DICE>), grid, dim3(NT), 0, st, logits, labels, weight, coef, grad_out, (const float*)w.nll, (const float*)w.rec, dlogits, C, S, groups);
    else CBIM_LAUNCH((k_topk_bwd<CMAX, 1, DICE>), grid, dim3(NT), 0, st, logits, labels, weight, coef, grad_out, (const float*)w.nll, (const float*)w.rec, dlogits, C, S, groups);
  }
}

static inline int topk_stream_grid(int64_t quads) {
  int64_t b = (quads + NT * 4 - 1) / (NT * 4);          // four 16-byte loads per thread
  if (b > TK_SUMS) b = TK_SUMS;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace cbim

using namespace cbim;

extern "C" size_t cbim_topk_workspace(int N, int C, int64_t S) {
  if (N < 1 || S < 1 || C < 1 || C > CMAX) return 0;
  return topk_layout(nullptr, N, C, S).bytes;
}

#define TOPK_CHECK_SHAPE()                                                                                              \
  CBIM_CHECK(N >= 1 && S >= 1, CBIM_EINVAL, "empty loss input (N %d, S %lld)", N, (long long)S);                        \
  CBIM_CHECK(C >= 1 && C <= CMAX, CBIM_EUNSUPPORTED, "loss supports up to %d classes (got %d)", CMAX, C);               \
  CBIM_CHECK((int64_t)N * S <= ((int64_t)1 << 31), CBIM_EUNSUPPORTED, "top-k loss takes up to 2^31 voxels (got %lld)",  \
             (long long)((int64_t)N * S))

extern "C" int cbim_topk_fwd(const float* logits, const int64_t* labels, const float* weight, int64_t K, int with_dice,
                             int N, int C, int64_t S, float* out, float* coef, void* workspace, size_t ws_bytes,
                             void* stream) {
  CBIM_CHECK(logits && labels && out && (coef || !with_dice), CBIM_EINVAL, "null argument");
  TOPK_CHECK_SHAPE();
  const int64_t total = (int64_t)N * S;
  CBIM_CHECK(K >= 1 && K <= total, CBIM_EINVAL, "top-k loss keeps 1..%lld voxels (got K = %lld)", (long long)total, (long long)K);
  const size_t need = cbim_topk_workspace(N, C, S);
  CBIM_CHECK(workspace && ws_bytes >= need, CBIM_EWORKSPACE, "loss workspace %zu < %zu", ws_bytes, need);
  CBIM_CHECK(((size_t)workspace & 15) == 0, CBIM_EINVAL, "loss workspace is not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const TopkWs w = topk_layout(workspace, N, C, S);
  const int V = loss_vec(logits, S, C);
  const int64_t groups = total / V;
  int nb = loss_blocks(total);                        // the grid of cbim_dice_ce_fwd: the Dice sums come out bit-equal
  if ((int64_t)nb * NT > groups) nb = (int)((groups + NT - 1) / NT);
  if (nb < 1) nb = 1;
  const unsigned rank = (unsigned)(total - K);        // ascending rank of the K-th largest value
  if (with_dice) topk_launch_fwd<true>(C, V, nb, st, logits, labels, weight, S, groups, w, rank, (unsigned)total);
  else topk_launch_fwd<false>(C, V, nb, st, logits, labels, weight, S, groups, w, rank, (unsigned)total);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  const int64_t quads = total / 4;
  const int tail = (int)(total - 4 * quads);
  const int ng = topk_stream_grid(quads);
  for (int pass = 0; pass < 4; ++pass) {
    CBIM_LAUNCH(k_topk_hist, dim3(ng), dim3(NT), 0, st, (const float*)w.nll, quads, tail, pass, w.hist);
    if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
    CBIM_LAUNCH(k_topk_pick, dim3(1), dim3(NT), 0, st, w.hist, pass, w.rec);
    if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  }
  CBIM_LAUNCH(k_topk_sum, dim3(ng), dim3(NT), 0, st, (const float*)w.nll, quads, tail, (const float*)w.rec, w.sums);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  if (with_dice) CBIM_LAUNCH(k_topk_finalize<true>, dim3(1), dim3(NT), 0, st, (const float*)w.partials, nb, C, (const double*)w.sums, ng, (const unsigned*)w.state, (double)K, w.rec, out, coef);
  else CBIM_LAUNCH(k_topk_finalize<false>, dim3(1), dim3(NT), 0, st, (const float*)w.partials, nb, C, (const double*)w.sums, ng, (const unsigned*)w.state, (double)K, w.rec, out, coef);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_topk_bwd(const float* logits, const int64_t* labels, const float* weight, const float* coef,
                             const float* grad_out, float* dlogits, int with_dice, int N, int C, int64_t S,
                             const void* workspace, void* stream) {
  CBIM_CHECK(logits && labels && grad_out && dlogits && workspace && (coef || !with_dice), CBIM_EINVAL, "null argument");
  TOPK_CHECK_SHAPE();
  CBIM_CHECK(((size_t)workspace & 15) == 0, CBIM_EINVAL, "loss workspace is not 16-byte aligned");
  const int64_t total = (int64_t)N * S;
  const TopkWs w = topk_layout((void*)workspace, N, C, S);
  int V = loss_vec(logits, S, C);
  if (V > 1 && ((size_t)dlogits % (V * 4)) != 0) V = 1;
  const int64_t groups = total / V;
  int64_t b = (groups + NT - 1) / NT;
  if (b > 256 * 16) b = 256 * 16;
  if (b < 1) b = 1;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)b);
  if (with_dice) topk_launch_bwd<true>(C, V, grid, st, logits, labels, weight, coef, grad_out, w, dlogits, S, groups);
  else topk_launch_bwd<false>(C, V, grid, st, logits, labels, weight, coef, grad_out, w, dlogits, S, groups);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

CBIM_DEFINE_WARM(topk)
