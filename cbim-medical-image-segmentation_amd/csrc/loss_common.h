// loss_common.h — what the loss kernel files share (loss_kernels.hip: CE + Dice, focal_kernels.hip: focal [+ Dice]):
// the vector access of V consecutive voxels, the launch geometry, the fixed-order fp64 reduction of the workgroup
// partials and the per-class Dice arithmetic.  ONE definition of each, so the Dice term of either family is the same
// number bit for bit (tests/focal_checks.py compares them with torch.equal).
#pragma once
#include "cbim_common.h"

namespace cbim {

static constexpr int NT = 256;
static constexpr int CMAX = 32;
static constexpr float SMOOTH = 1e-5f;

// V consecutive voxels per thread: every class plane is read with one V*4-byte load per lane (16 B for V = 4, a
// wave instruction then covers 1 KiB of one plane), labels as V int64.  CT = compile-time class bound (C <= CT) so
// the per-class arrays live in registers without predicated dead work (C = 16 ran the CT = 32 loops before).
template <int V> struct VecF;
template <> struct VecF<4> { typedef f32x4 type; };
template <> struct VecF<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct VecF<1> { typedef float type; };
template <int V> __device__ __forceinline__ void ldv(const float* p, float* o) {
  typename VecF<V>::type q = *(const typename VecF<V>::type*)p;
  if constexpr (V == 1) o[0] = q;
  else {
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = q[i];
  }
}
template <int V> __device__ __forceinline__ void stv(float* p, const float* o) {
  typename VecF<V>::type q;
  if constexpr (V == 1) q = o[0];
  else {
#pragma unroll
    for (int i = 0; i < V; ++i) q[i] = o[i];
  }
  *(typename VecF<V>::type*)p = q;
}

// The finalize kernels' reduction of `nblk` workgroup records of `nv` floats each into tot[nv] (fp64, fixed order):
// 4 thread groups stride over the records (independent loads in flight), fixed-order merge.  Called by all NT threads
// of the single workgroup; tot is valid after the call.
__device__ __forceinline__ void loss_reduce_partials(const float* __restrict__ partials, int nblk, int nv,
                                                     double* tot, double (*part)[3 * CMAX + 3]) {
  {
    const int li = threadIdx.x & 63, pg = threadIdx.x >> 6;
    for (int i = li; i < nv; i += 64) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;   // 4 loads in flight per trip
      int b = pg;
      for (; b + 12 < nblk; b += 16) {
        a0 += (double)partials[(size_t)b * nv + i];
        a1 += (double)partials[(size_t)(b + 4) * nv + i];
        a2 += (double)partials[(size_t)(b + 8) * nv + i];
        a3 += (double)partials[(size_t)(b + 12) * nv + i];
      }
      for (; b < nblk; b += 4) a0 += (double)partials[(size_t)b * nv + i];
      part[pg][i] = (a0 + a1) + (a2 + a3);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nv; i += NT) tot[i] = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
  __syncthreads();
}

// Class c of the Dice loss from its three sums (loss_kernels.hip header): writes the backward coefficients
// coef[c] = dL/dTP_c, coef[C + c] = dL/dSP_c and the per-class term coef[2C + 1 + c]; returns 1 - dice_c.
__device__ __forceinline__ double dice_class_term(double TP, double SP, double CNT, int C, int c,
                                                  float* __restrict__ coef) {
  double eps = (double)SMOOTH;
  double FP = SP - TP, FN = CNT - TP;
  double T = FP + FN + eps;
  double r = FP / T;
  bool open = (r >= 0.2 && r <= 0.8);
  double alpha = r < 0.2 ? 0.2 : (r > 0.8 ? 0.8 : r);
  double den = TP + alpha * FP + (1.0 - alpha) * FN;
  double dice = TP / (den + eps);
  // d alpha / d TP, d alpha / d SP (only inside the clamp)
  double da_dTP = open ? (FP - FN - eps) / (T * T) : 0.0;
  double da_dSP = open ? (FN + eps) / (T * T) : 0.0;
  double dden_dTP = (SP - CNT) * da_dTP;            // the explicit TP terms cancel
  double dden_dSP = alpha + (SP - CNT) * da_dSP;
  double q = TP / ((den + eps) * (den + eps));
  double ddice_dTP = 1.0 / (den + eps) - q * dden_dTP;
  double ddice_dSP = -q * dden_dSP;
  coef[c] = (float)(-ddice_dTP / C);
  coef[C + c] = (float)(-ddice_dSP / C);
  coef[2 * C + 1 + c] = (float)(1.0 - dice);        // per-class loss term: DiceLoss(reduce=False) (losses.py:48-50)
  return 1.0 - dice;
}

static inline int loss_blocks(int64_t total) {
  int64_t b = (total + NT * 8 - 1) / (NT * 8);   // upper bound over the vector widths (groups <= total)
  // four workgroups per CU (16 waves: one 64-register wave per SIMD left the loads latency-bound, 55 us for 151 MB at
  // 1x16x128^3); the single-workgroup finalize kernel walks these records, four independent loads per thread and trip
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (int)b;
}

// voxels per thread: 4 (C <= 16) / 2 (C <= 32) consecutive voxels when every class plane stays aligned for the
// vector load (S a multiple of V, base pointer aligned); otherwise one voxel per thread
static inline int loss_vec(const void* logits, int64_t S, int C) {
  const int V = C <= 16 ? 4 : 2;
  if (S % V != 0 || ((size_t)logits % (V * 4)) != 0) return 1;
  return V;
}

}  // namespace cbim
