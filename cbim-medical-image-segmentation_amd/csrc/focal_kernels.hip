// focal_kernels.hip — focal loss, optionally fused with the soft Dice loss of loss_kernels.hip, in one pass over the logits.
//
// Reference: FocalLoss (/root/reference/training/losses.py:60-98) [+ DiceLoss (:8-58)].  The reference materialises
// softmax, log-softmax, the one-hot mask and two products; here the logits are read ONCE in the forward and once in the
// backward, like the CE + Dice kernels whose structure (V voxels per thread, CT class bound, fixed-order workgroup
// partials, single-workgroup fp64 finalize: loss_common.h) this file follows.
//
// Per voxel, with e_c = exp(z_c - max), se = sum_c e_c, y the label, a = alpha[y] (1 without a table):
//   p = e_y / se,   q = (sum_{c != y} e_c) / se  (NOT 1 - p: exact where p -> 1),   log p = z_y - max - log se
//   L = -a q^g log p,      dL/dz_c = K (delta_cy - p_c),   K = a (g p q^(g-1) log p - q^g)
// g = 0 is the plain -a log p with K = -a; g = 1, 2, 3 are products (no transcendental); other g go through powf, and
// q = 0 gives loss 0 and K = 0 for every g > 0 (the reference's autograd has 0 * inf = NaN there for 0 < g < 1).
// A label outside [0, C) is never used as an index: the voxel adds nothing to the focal sum, TP or CNT and is counted.
#include "loss_common.h"

namespace cbim {

// (q^g, q^(g-1)) for q in [0, 1]; `mode` is wave-uniform: 0 -> g = 0, 1..3 -> that integer, 4 -> powf.  POW (mode 4) is a
// template parameter of the kernels: the instantiations that serve g = 0, 1, 2, 3 carry no powf code or registers.
template <bool POW>
__device__ __forceinline__ void focal_pow(float q, float gamma, int mode, float& qg, float& qg1) {
  if constexpr (POW) {
    if (q > 0.f) { qg1 = powf(q, gamma - 1.f); qg = qg1 * q; }
    else { qg = 0.f; qg1 = 0.f; }
  } else {
    if (mode == 0) { qg = 1.f; qg1 = 0.f; }              // qg1 is multiplied by g = 0
    else if (mode == 1) { qg = q; qg1 = 1.f; }
    else if (mode == 2) { qg = q * q; qg1 = q; }
    else { qg1 = q * q; qg = qg1 * q; }
  }
}
static inline int focal_mode(float gamma) {
  return gamma == 0.f ? 0 : gamma == 1.f ? 1 : gamma == 2.f ? 2 : gamma == 3.f ? 3 : 4;
}

// partial layout per workgroup: DICE: [3*C + 2] = TP[C], SP[C], CNT[C], focal sum, #labels outside [0, C);  else [2].
// The TP / SP / CNT accumulation is that of k_dice_ce_fwd statement for statement (same p_c, same order, same grid).
// (second launch bound: the waves per SIMD the four-voxel kernels are held to, those of their CE + Dice siblings)
template <int CT, int V, bool DICE, bool POW>
__global__ void __launch_bounds__(NT, (CT == 16 && V == 4 && !POW ? 3 : 1)) k_focal_fwd(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                  const float* __restrict__ alpha, float gamma, int mode, int C,
                                                  int64_t S, int64_t groups, float* __restrict__ partials) {
  constexpr int CA = DICE ? CT : 1;
  float tp[CA], sp[CA], cnt[CA];
#pragma unroll
  for (int c = 0; c < CA; ++c) { tp[c] = 0.f; sp[c] = 0.f; cnt[c] = 0.f; }
  float fsum = 0.f, bad = 0.f;
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < groups; g += (int64_t)gridDim.x * NT) {
    const int64_t r = g * V;
    const int64_t n = r / S, v = r % S;
    const float* zp = z + (size_t)n * C * S + v;
    int lab[V];
#pragma unroll
    for (int i = 0; i < V; ++i) lab[i] = (int)y[r + i];
    float l[CT][V];
    float mx[V], zy[V], se[V], so[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = -INFINITY; zy[i] = 0.f; se[i] = 0.f; so[i] = 0.f; }
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
        for (int i = 0; i < V; ++i) {
          l[c][i] = __expf(l[c][i] - mx[i]);
          se[i] += l[c][i];
          so[i] += c == lab[i] ? 0.f : l[c][i];
        }
      }
    float inv[V];
#pragma unroll
    for (int i = 0; i < V; ++i) inv[i] = 1.f / se[i];
    if constexpr (DICE) {
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
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const bool ok = (unsigned)lab[i] < (unsigned)C;
      const float a = ok ? (alpha ? alpha[lab[i]] : 1.f) : 0.f;
      const float logp = zy[i] - mx[i] - __logf(se[i]);
      float qg, qg1;
      focal_pow<POW>(so[i] * inv[i], gamma, mode, qg, qg1);
      fsum += ok ? -a * qg * logp : 0.f;
      bad += ok ? 0.f : 1.f;
    }
  }
  // workgroup reduction (fixed order): wave shuffles then 4 waves through LDS
  constexpr int NR = DICE ? 3 * CT + 2 : 2;
  constexpr int FO = DICE ? 3 * CT : 0;               // where the focal sum and the count sit in a wave's row
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
    float a = wave_sum(fsum), e = wave_sum(bad);
    if (lane == 0) { red[wave][FO] = a; red[wave][FO + 1] = e; }
  }
  __syncthreads();
  const int nd = DICE ? 3 * C : 0;
  float* out = partials + (size_t)blockIdx.x * (nd + 2);
  for (int i = threadIdx.x; i < nd + 2; i += NT) {
    int src = i < nd ? (i / C) * CT + (i % C) : FO + (i - nd);
    out[i] = red[0][src] + red[1][src] + red[2][src] + red[3][src];
  }
}

// single workgroup: reduce partials in fp64; out = (focal sum, focal mean over `count` voxels, Dice, #bad labels, mean + Dice).
// DICE: coef as k_dice_ce_finalize leaves it ([2][C] class coefficients, [C] per-class terms at 2C + 1); coef[2C] = 1/count.
template <bool DICE>
__global__ void __launch_bounds__(NT) k_focal_finalize(const float* __restrict__ partials, int nblk, int C, double count,
                                                       float* __restrict__ out, float* __restrict__ coef) {
  __shared__ double tot[3 * CMAX + 3];
  __shared__ double part[4][3 * CMAX + 3];
  __shared__ double dice_term[CMAX];
  const int nd = DICE ? 3 * C : 0;
  loss_reduce_partials(partials, nblk, nd + 2, tot, part);
  if constexpr (DICE) {
    if ((int)threadIdx.x < C) {
      int c = threadIdx.x;
      dice_term[c] = dice_class_term(tot[c], tot[C + c], tot[2 * C + c], C, c, coef);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double dl = 0.0;
    if constexpr (DICE) {
      for (int c = 0; c < C; ++c) dl += dice_term[c];
      dl /= C;
      coef[2 * C] = (float)(1.0 / count);
    }
    const float fmean = (float)(tot[nd] / count), fdice = (float)dl;
    out[0] = (float)tot[nd];
    out[1] = fmean;
    out[2] = fdice;
    out[3] = (float)tot[nd + 1];   // labels outside [0, C)
    out[4] = fmean + fdice;        // the float32 sum of the two entries, as adding them on the host side would give
  }
}

// dlogits = g_focal * dFocalSum/dz [+ g_dice * dDice/dz]   (grad_out = {g_focal per voxel, g_dice} on the device)
template <int CT, int V, bool DICE, bool POW>
__global__ void __launch_bounds__(NT, (CT == 16 && V == 4 && !POW ? 4 : 1)) k_focal_bwd(const float* __restrict__ z, const int64_t* __restrict__ y,
                                                  const float* __restrict__ alpha, const float* __restrict__ coef,
                                                  const float* __restrict__ grad_out, float* __restrict__ dz,
                                                  float gamma, int mode, int C, int64_t S, int64_t groups) {
  __shared__ float cf[2 * CMAX];
  if constexpr (DICE) {
    if ((int)threadIdx.x < 2 * C) cf[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
  }
  const float g_focal = grad_out[0], g_dice = DICE ? grad_out[1] : 0.f;
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < groups; g += (int64_t)gridDim.x * NT) {
    const int64_t r = g * V;
    const int64_t n = r / S, v = r % S;
    const float* zp = z + (size_t)n * C * S + v;
    float* dp = dz + (size_t)n * C * S + v;
    int lab[V];
#pragma unroll
    for (int i = 0; i < V; ++i) lab[i] = (int)y[r + i];
    float l[CT][V];
    float mx[V], zy[V], se[V], so[V], ey[V], dot[V], K[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = -INFINITY; zy[i] = 0.f; se[i] = 0.f; so[i] = 0.f; ey[i] = 0.f; dot[i] = 0.f; }
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
        for (int i = 0; i < V; ++i) {
          l[c][i] = __expf(l[c][i] - mx[i]);
          se[i] += l[c][i];
          if (c == lab[i]) ey[i] = l[c][i]; else so[i] += l[c][i];
        }
      }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const bool ok = (unsigned)lab[i] < (unsigned)C;     // see k_focal_fwd: such a voxel only feeds SP
      const float a = ok ? (alpha ? alpha[lab[i]] : 1.f) : 0.f;
      const float logp = zy[i] - mx[i] - __logf(se[i]);
      se[i] = 1.f / se[i];
      float qg, qg1;
      focal_pow<POW>(so[i] * se[i], gamma, mode, qg, qg1);
      const float k = mode == 0 ? -a : a * (gamma * (ey[i] * se[i]) * qg1 * logp - qg);
      K[i] = ok ? g_focal * k : 0.f;
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
            o[i] = K[i] * ((c == lab[i] ? 1.f : 0.f) - l[c][i]) + g_dice * d_dice;
          }
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] = K[i] * ((c == lab[i] ? 1.f : 0.f) - l[c][i]);
        }
        stv<V>(dp + (size_t)c * S, o);
      }
  }
}

template <bool DICE, bool POW>
static void focal_launch_fwd(int C, int V, int nb, hipStream_t st, const float* logits, const int64_t* labels,
                             const float* alpha, float gamma, int mode, int64_t S, int64_t groups, float* ws) {
  if (C <= 16) {
    if (V == 4) CBIM_LAUNCH((k_focal_fwd<16, 4, DICE, POW>), dim3(nb), dim3(NT), 0, st, logits, labels, alpha, gamma, mode, C, S, groups, ws);
    else CBIM_LAUNCH((k_focal_fwd<16, 1, DICE, POW>), dim3(nb), dim3(NT), 0, st, logits, labels, alpha, gamma, mode, C, S, groups, ws);
  } else {
    if (V == 2) CBIM_LAUNCH((k_focal_fwd<CMAX, 2, DICE, POW>), dim3(nb), dim3(NT), 0, st, logits, labels, alpha, gamma, mode, C, S, groups, ws);
    else CBIM_LAUNCH((k_focal_fwd<CMAX, 1, DICE, POW>), dim3(nb), dim3(NT), 0, st, logits, labels, alpha, gamma, mode, C, S, groups, ws);
  }
}

template <bool DICE, bool POW>
static void focal_launch_bwd(int C, int V, dim3 grid, hipStream_t st, const float* logits, const int64_t* labels,
                             const float* alpha, const float* coef, const float* grad_out, float* dlogits, float gamma,
                             int mode, int64_t S, int64_t groups) {
  if (C <= 16) {
    if (V == 4) CBIM_LAUNCH((k_focal_bwd<16, 4, DICE, POW>), grid, dim3(NT), 0, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, C, S, groups);
    else CBIM_LAUNCH((k_focal_bwd<16, 1, DICE, POW>), grid, dim3(NT), 0, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, C, S, groups);
  } else {
    if (V == 2) CBIM_LAUNCH((k_focal_bwd<CMAX, 2, DICE, POW>), grid, dim3(NT), 0, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, C, S, groups);
    else CBIM_LAUNCH((k_focal_bwd<CMAX, 1, DICE, POW>), grid, dim3(NT), 0, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, C, S, groups);
  }
}

}  // namespace cbim

using namespace cbim;

extern "C" size_t cbim_focal_workspace(int N, int C, int64_t S) {
  return (size_t)loss_blocks((int64_t)N * S) * (3 * C + 2) * sizeof(float);
}

extern "C" int cbim_focal_fwd(const float* logits, const int64_t* labels, const float* alpha, float gamma,
                              int with_dice, int N, int C, int64_t S, float* out, float* coef, void* workspace,
                              size_t ws_bytes, void* stream) {
  CBIM_CHECK(logits && labels && out && (coef || !with_dice), CBIM_EINVAL, "null argument");
  CBIM_CHECK(gamma >= 0.f && gamma < INFINITY, CBIM_EINVAL, "focal gamma must be a finite number >= 0 (got %g)", (double)gamma);
  CBIM_CHECK(N >= 1 && S >= 1, CBIM_EINVAL, "empty loss input (N %d, S %lld)", N, (long long)S);
  CBIM_CHECK(C >= 1 && C <= CMAX, CBIM_EUNSUPPORTED, "loss supports up to %d classes (got %d)", CMAX, C);
  size_t need = cbim_focal_workspace(N, C, S);
  CBIM_CHECK(workspace && ws_bytes >= need, CBIM_EWORKSPACE, "loss workspace %zu < %zu", ws_bytes, need);
  int64_t total = (int64_t)N * S;
  hipStream_t st = (hipStream_t)stream;
  const int V = loss_vec(logits, S, C);
  const int64_t groups = total / V;
  int nb = loss_blocks(total);                        // the grid of cbim_dice_ce_fwd: the Dice sums come out bit-equal
  if ((int64_t)nb * NT > groups) nb = (int)((groups + NT - 1) / NT);
  if (nb < 1) nb = 1;
  float* ws = (float*)workspace;
  const int mode = focal_mode(gamma);
  if (with_dice && mode == 4) focal_launch_fwd<true, true>(C, V, nb, st, logits, labels, alpha, gamma, mode, S, groups, ws);
  else if (with_dice) focal_launch_fwd<true, false>(C, V, nb, st, logits, labels, alpha, gamma, mode, S, groups, ws);
  else if (mode == 4) focal_launch_fwd<false, true>(C, V, nb, st, logits, labels, alpha, gamma, mode, S, groups, ws);
  else focal_launch_fwd<false, false>(C, V, nb, st, logits, labels, alpha, gamma, mode, S, groups, ws);
  if (CBIM_LAST_LAUNCH() != hipSuccess) return CBIM_ELAUNCH;
  if (with_dice) CBIM_LAUNCH(k_focal_finalize<true>, dim3(1), dim3(NT), 0, st, (const float*)workspace, nb, C, (double)total, out, coef);
  else CBIM_LAUNCH(k_focal_finalize<false>, dim3(1), dim3(NT), 0, st, (const float*)workspace, nb, C, (double)total, out, coef);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_focal_bwd(const float* logits, const int64_t* labels, const float* alpha, const float* coef,
                              const float* grad_out, float* dlogits, float gamma, int with_dice, int N, int C,
                              int64_t S, void* stream) {
  CBIM_CHECK(logits && labels && grad_out && dlogits && (coef || !with_dice), CBIM_EINVAL, "null argument");
  CBIM_CHECK(gamma >= 0.f && gamma < INFINITY, CBIM_EINVAL, "focal gamma must be a finite number >= 0 (got %g)", (double)gamma);
  CBIM_CHECK(N >= 1 && S >= 1, CBIM_EINVAL, "empty loss input (N %d, S %lld)", N, (long long)S);
  CBIM_CHECK(C >= 1 && C <= CMAX, CBIM_EUNSUPPORTED, "loss supports up to %d classes (got %d)", CMAX, C);
  int64_t total = (int64_t)N * S;
  int V = loss_vec(logits, S, C);
  if (V > 1 && ((size_t)dlogits % (V * 4)) != 0) V = 1;
  const int64_t groups = total / V;
  int64_t b = (groups + NT - 1) / NT;
  if (b > 256 * 16) b = 256 * 16;
  if (b < 1) b = 1;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)b);
  const int mode = focal_mode(gamma);
  if (with_dice && mode == 4) focal_launch_bwd<true, true>(C, V, grid, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, S, groups);
  else if (with_dice) focal_launch_bwd<true, false>(C, V, grid, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, S, groups);
  else if (mode == 4) focal_launch_bwd<false, true>(C, V, grid, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, S, groups);
  else focal_launch_bwd<false, false>(C, V, grid, st, logits, labels, alpha, coef, grad_out, dlogits, gamma, mode, S, groups);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

CBIM_DEFINE_WARM(focal)
