// optim_kernels.hip — multi-tensor AdamW (+ optional EMA of the weights) in ONE launch.
//
// Replaces, per training iteration, torch.optim.AdamW(..., eps=1e-5).step() (/root/reference/training/utils.py:14,
// called at train.py:216) and update_ema_variables (training/utils.py:98-105, train.py:217-218): 45-278 tensors,
// several elementwise launches each in the eager path -> one streaming kernel, 16 bytes/parameter read
// (p, g, m, v [, ema]) and written (p, m, v [, ema]).  HBM-bound.
//
// hyper (device float[10]) = {step, lr, beta1, beta2, eps, weight_decay, ema_alpha, max_grad_norm, 1-beta1, 1-beta2} (the
// last two rounded from double on the host, as torch does): the step counter lives on
// the device (k_optim_tick) so the whole update is capturable in a hipGraph; the host only rewrites hyper[1]
// when the scheduler changes the learning rate.  hyper[7] is read by the guarded step alone (k_grad_ctl).
//
// The guarded step (cbim_adamw_ema_step_guarded) adds what a real run does around optimizer.step(): clipping by the global
// gradient norm (torch.nn.utils.clip_grad_norm_), the unscale of torch.amp.GradScaler and the skip of a step whose gradients
// are not finite — k_grad_sumsq + k_grad_ctl + the guarded form of k_adamw_ema, one more read of the gradients (4 bytes per
// parameter), no rewrite of them and no host round trip.
//   AdamW (decoupled decay, torch semantics):  p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
//     p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
//   EMA: a = min(1 - 1/t, alpha)  (global_step = t-1 in the reference's numbering);  ema = a*ema + (1-a)*p_new
#include "cbim_common.h"

namespace cbim {

static constexpr int ONT = 256;
static constexpr int OCHUNK = 4096;   // parameters per workgroup

__global__ void k_optim_tick(float* hyper) {
  if (threadIdx.x == 0 && blockIdx.x == 0) hyper[0] += 1.0f;
}

// GUARD = false is the step as it always was.  GUARD = true (cbim_adamw_ema_step_guarded) leaves at once when k_grad_ctl set
// ctl.skip — parameters, moments and the EMA copy stay untouched — and otherwise uses g * ctl.mult (unscale and clip in one
// factor) wherever the plain step uses g.  The clipped gradient is NOT written back: p.grad keeps what backward produced.
template <bool GUARD>
__device__ __forceinline__ void adamw_ema_body(const cbim_optim_tensor* __restrict__ tab, const int32_t* __restrict__ blk_tensor,
                                               const int32_t* __restrict__ blk_chunk, const float* __restrict__ hyper,
                                               const float* __restrict__ ctl) {
  float mult = 1.f;
  if (GUARD) {
    if (ctl[2] != 0.f) return;
    mult = ctl[1];
  }
  const cbim_optim_tensor t = tab[blk_tensor[blockIdx.x]];
  const int64_t base = (int64_t)blk_chunk[blockIdx.x] * OCHUNK;
  const float step = hyper[0], lr = hyper[1], b1 = hyper[2], b2 = hyper[3], eps = hyper[4], wd = hyper[5];
  const float alpha_max = hyper[6], omb1 = hyper[8], omb2 = hyper[9];
  const float bc1 = 1.f - powf(b1, step), bc2s = sqrtf(1.f - powf(b2, step));
  const float step_size = lr / bc1, decay = 1.f - lr * wd;
  float a = 1.f - 1.f / step;
  if (a > alpha_max) a = alpha_max;
  float* p = (float*)t.p;
  const float* g = (const float*)t.g;
  float* m = (float*)t.m;
  float* v = (float*)t.v;
  float* e = (float*)t.ema;
  for (int i = threadIdx.x; i < OCHUNK; i += ONT) {
    int64_t k = base + i;
    if (k >= t.numel) break;
    float gv = GUARD ? g[k] * mult : g[k], pv = p[k] * decay;
    float mv = b1 * m[k] + omb1 * gv;
    float vv = b2 * v[k] + omb2 * gv * gv;
    pv -= step_size * mv / (sqrtf(vv) / bc2s + eps);
    p[k] = pv; m[k] = mv; v[k] = vv;
    if (e) e[k] = a * e[k] + (1.f - a) * pv;
  }
}

__global__ void __launch_bounds__(ONT) k_adamw_ema(const cbim_optim_tensor* __restrict__ tab,
                                                   const int32_t* __restrict__ blk_tensor,
                                                   const int32_t* __restrict__ blk_chunk,
                                                   const float* __restrict__ hyper) {
  adamw_ema_body<false>(tab, blk_tensor, blk_chunk, hyper, nullptr);
}

__global__ void __launch_bounds__(ONT) k_adamw_ema_guarded(const cbim_optim_tensor* __restrict__ tab,
                                                           const int32_t* __restrict__ blk_tensor,
                                                           const int32_t* __restrict__ blk_chunk,
                                                           const float* __restrict__ hyper, const float* __restrict__ ctl) {
  adamw_ema_body<true>(tab, blk_tensor, blk_chunk, hyper, ctl);
}

// ---- global gradient norm, clip coefficient and the skip decision ---------------------------------------------------------
// k_grad_sumsq: workgroup b writes partial[b] = sum over its chunk of (g * inv_scale)^2, inv_scale = 1 / *grad_scale (1 when the
// pointer is null).  The gradient is unscaled BEFORE it is squared: a 2^16-scaled value whose square leaves fp32 range is still a
// finite gradient.  An inf or NaN element makes the partial, and so the norm, non-finite by itself.
// The order of the sum is a function of the element's index in the chunk alone: thread t owns the groups of four elements
// q = t, t + 256, ... (16 elements of a full chunk) and adds their squares in index order, then the xor butterfly over the wave,
// then the four waves in wave order from LDS.  No atomics: the same gradients give the same bits on every run and every replica.
// A chunk that starts on a 16-byte boundary is read as float4; any other 4-byte aligned start (a view into a flat all-reduce
// bucket) is read element by element with the SAME ownership, so the sum does not depend on the alignment; the last, partial
// group of a chunk is read element by element in both forms.
// Roundings on the longest path to partial[b]: 3 in a square (unscale counts twice, the product once), 15 additions in the
// thread, 6 in the butterfly, 3 across the waves = 27; k_grad_ctl adds in double.
__global__ void __launch_bounds__(ONT) k_grad_sumsq(const cbim_optim_tensor* __restrict__ tab, const int32_t* __restrict__ blk_tensor,
                                                    const int32_t* __restrict__ blk_chunk, const float* __restrict__ grad_scale,
                                                    float* __restrict__ partial) {
  __shared__ float s_wave[ONT / 64];
  const cbim_optim_tensor t = tab[blk_tensor[blockIdx.x]];
  const int64_t base = (int64_t)blk_chunk[blockIdx.x] * OCHUNK;
  const float inv = grad_scale ? 1.f / grad_scale[0] : 1.f;
  const int64_t left = t.numel - base;
  const int n = left < OCHUNK ? (int)left : OCHUNK;          // 1..OCHUNK elements of this chunk
  const float* g = (const float*)t.g + base;
  const bool vec = (((uintptr_t)g) & 15) == 0;
  float acc = 0.f;
  if (vec && n == OCHUNK) {                                  // the common case: all four loads in flight before the first add
    f32x4 w[OCHUNK / (4 * ONT)];
#pragma unroll
    for (int j = 0; j < OCHUNK / (4 * ONT); ++j) w[j] = *(const f32x4*)(g + 4 * (threadIdx.x + j * ONT));
#pragma unroll
    for (int j = 0; j < OCHUNK / (4 * ONT); ++j) {
      const float x[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float u = x[c] * inv;
        acc += u * u;
      }
    }
  } else for (int q = threadIdx.x; 4 * q < n; q += ONT) {    // same elements, same order
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && 4 * q + 4 <= n) {
      const f32x4 w = *(const f32x4*)(g + 4 * q);
      x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * q + c < n) x[c] = g[4 * q + c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float u = x[c] * inv;
      acc += u * u;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = s_wave[0];
    for (int w = 1; w < ONT / 64; ++w) s += s_wave[w];
    partial[blockIdx.x] = s;
  }
}

// k_grad_ctl: ONE workgroup.  Adds partial[0..nblocks) in double in a fixed order (thread t takes t, t + 256, ...; then a
// tree over the 256 threads), and writes the control block ctl = {norm, mult, skip, skipped}:
//   norm    = sqrt(total), the L2 norm of the unscaled gradients
//   mult    = inv_scale * min(1, max_norm / (norm + 1e-6))   (clip_grad_norm_'s coefficient, fp32 as torch computes it);
//             max_norm = hyper[7] <= 0, inf or NaN means "do not clip": the coefficient is then exactly 1
//   skip    = 1 when norm is not finite or *found_inf > 0, else 0;   skipped += skip
// and ticks the step counter hyper[0] only when skip == 0 (this replaces k_optim_tick on the guarded path).
// hyper == nullptr (cbim_grad_norm): only ctl[0] = norm is written.
__global__ void __launch_bounds__(ONT) k_grad_ctl(const float* __restrict__ partial, int nblocks, float* hyper, float* ctl,
                                                  const float* __restrict__ grad_scale, const float* __restrict__ found_inf) {
  __shared__ double s_sum[ONT];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += ONT) s += (double)partial[i];
  s_sum[threadIdx.x] = s;
  __syncthreads();
  for (int o = ONT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(s_sum[0]);
  ctl[0] = norm;
  if (!hyper) return;
  const float inv = grad_scale ? 1.f / grad_scale[0] : 1.f;
  const float max_norm = hyper[7];
  float coef = 1.f;
  if (max_norm > 0.f && max_norm <= 3.402823466e38f) {
    coef = max_norm / (norm + 1e-6f);
    if (!(coef < 1.f)) coef = 1.f;
  }
  const bool finite = norm <= 3.402823466e38f;                // false for inf and for NaN
  const bool skip = !finite || (found_inf && found_inf[0] > 0.f);
  ctl[1] = inv * coef;
  ctl[2] = skip ? 1.f : 0.f;
  ctl[3] += skip ? 1.f : 0.f;
  if (!skip) hyper[0] += 1.0f;
}

// update_ema_variables alone (training/utils.py:98-102), for callers that keep torch's optimizer:
// ema = a*ema + (1-a)*p over every tensor of the table in one launch (records use .p and .ema only).
__global__ void __launch_bounds__(ONT) k_ema(const cbim_optim_tensor* __restrict__ tab, const int32_t* __restrict__ blk_tensor,
                                             const int32_t* __restrict__ blk_chunk, float a, float oma) {
  const cbim_optim_tensor t = tab[blk_tensor[blockIdx.x]];
  const int64_t base = (int64_t)blk_chunk[blockIdx.x] * OCHUNK;
  const float* p = (const float*)t.p;
  float* e = (float*)t.ema;
  for (int i = threadIdx.x; i < OCHUNK; i += ONT) {
    int64_t k = base + i;
    if (k >= t.numel) break;
    e[k] = fmaf(oma, p[k], e[k] * a);   // ema.mul_(alpha) rounds, .add_(param, alpha=1-alpha) is a fused multiply-add in ATen
  }
}

}  // namespace cbim

using namespace cbim;

extern "C" int cbim_optim_chunk(void) { return OCHUNK; }

extern "C" int cbim_adamw_ema_step(const cbim_optim_tensor* tensors, const int32_t* blk_tensor, const int32_t* blk_chunk,
                                   int nblocks, float* hyper, void* stream) {
  CBIM_CHECK(tensors && blk_tensor && blk_chunk && hyper && nblocks >= 1, CBIM_EINVAL, "adamw_ema_step: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  CBIM_LAUNCH(k_optim_tick, dim3(1), dim3(64), 0, st, hyper);
  CBIM_LAUNCH(k_adamw_ema, dim3(nblocks), dim3(ONT), 0, st, tensors, blk_tensor, blk_chunk, (const float*)hyper);
  hipError_t e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "adamw_ema_step launch: %s", hipGetErrorString(e));
  return CBIM_OK;
}

extern "C" int cbim_adamw_ema_step_guarded(const cbim_optim_tensor* tensors, const int32_t* blk_tensor, const int32_t* blk_chunk,
                                           int nblocks, float* hyper, float* partial, float* ctl, const float* grad_scale,
                                           const float* found_inf, void* stream) {
  CBIM_CHECK(tensors && blk_tensor && blk_chunk && hyper && partial && ctl && nblocks >= 1, CBIM_EINVAL,
             "adamw_ema_step_guarded: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  CBIM_LAUNCH(k_grad_sumsq, dim3(nblocks), dim3(ONT), 0, st, tensors, blk_tensor, blk_chunk, grad_scale, partial);
  hipError_t e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "adamw_ema_step_guarded launch (sumsq): %s", hipGetErrorString(e));
  CBIM_LAUNCH(k_grad_ctl, dim3(1), dim3(ONT), 0, st, (const float*)partial, nblocks, hyper, ctl, grad_scale, found_inf);
  e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "adamw_ema_step_guarded launch (ctl): %s", hipGetErrorString(e));
  CBIM_LAUNCH(k_adamw_ema_guarded, dim3(nblocks), dim3(ONT), 0, st, tensors, blk_tensor, blk_chunk, (const float*)hyper,
              (const float*)ctl);
  e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "adamw_ema_step_guarded launch: %s", hipGetErrorString(e));
  return CBIM_OK;
}

extern "C" int cbim_grad_norm(const cbim_optim_tensor* tensors, const int32_t* blk_tensor, const int32_t* blk_chunk, int nblocks,
                              float* partial, float* out, void* stream) {
  CBIM_CHECK(tensors && blk_tensor && blk_chunk && partial && out && nblocks >= 1, CBIM_EINVAL, "grad_norm: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  CBIM_LAUNCH(k_grad_sumsq, dim3(nblocks), dim3(ONT), 0, st, tensors, blk_tensor, blk_chunk, (const float*)nullptr, partial);
  hipError_t e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "grad_norm launch (sumsq): %s", hipGetErrorString(e));
  CBIM_LAUNCH(k_grad_ctl, dim3(1), dim3(ONT), 0, st, (const float*)partial, nblocks, (float*)nullptr, out, (const float*)nullptr,
              (const float*)nullptr);
  e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "grad_norm launch (ctl): %s", hipGetErrorString(e));
  return CBIM_OK;
}

extern "C" int cbim_ema_step(const cbim_optim_tensor* tensors, const int32_t* blk_tensor, const int32_t* blk_chunk,
                             int nblocks, float alpha, float one_minus_alpha, void* stream) {
  CBIM_CHECK(tensors && blk_tensor && blk_chunk && nblocks >= 1, CBIM_EINVAL, "ema_step: bad arguments");
  CBIM_LAUNCH(k_ema, dim3(nblocks), dim3(ONT), 0, (hipStream_t)stream, tensors, blk_tensor, blk_chunk, alpha, one_minus_alpha);
  hipError_t e = CBIM_LAST_LAUNCH();
  CBIM_CHECK(e == hipSuccess, CBIM_ELAUNCH, "ema_step launch: %s", hipGetErrorString(e));
  return CBIM_OK;
}

CBIM_DEFINE_WARM(optim)
