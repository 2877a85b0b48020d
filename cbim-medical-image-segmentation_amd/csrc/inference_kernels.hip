// inference_kernels.hip — sliding-window inference accumulation and evaluation Dice.
//
//   k_softmax_accumulate  inference_sliding_window's per-window tail (/root/reference/inference/inference3d.py:80-86):
//                         pred = softmax(net(window), 1); pred_output[window] += pred; counter[window] += 1
//                         — one pass over the window's logits instead of a softmax plus two strided slice-adds
//   k_prob_finalize       pred_output /= counter (:88), optionally with torch.max(pred, dim=1) of validation.py:44
//   k_dice_counts         calculate_dice (/root/reference/metric/utils.py:62-82): per block of `block` voxels the
//                         integer counts (pred==c & target==c, pred==c, target==c); the float32 sums the reference
//                         forms from 0/1 masks are these integers, so the host reproduces its arithmetic bit for bit
//   k_window_gather_mirror        the window slice + .contiguous() + one torch.flip per mirror variant of test-time
//                                 augmentation in one launch: V flipped copies of one window, stacked along the batch
//   k_softmax_accumulate_tta      k_softmax_accumulate over V mirror variants and an optional separable window weight:
//                                 every variant's logits are read once at the mirrored position, their softmaxes summed in
//                                 registers in variant order, and the accumulator gets ONE read-modify-write per class
//                                 (composed from torch: V flips of the logits, V accumulate launches, a multiply-add)
// All HBM-bound streaming kernels on NCDHW float32 probabilities (the layout the model head emits).
#include "cbim_common.h"
#include "gfx950_prims.h"

namespace cbim {

static constexpr int INT_ = 256;

__global__ void __launch_bounds__(INT_) k_softmax_accumulate(const float* __restrict__ logits, float* __restrict__ acc,
                                                             float* __restrict__ counter, int K, int wd, int wh, int ww,
                                                             int D, int H, int W, int d0, int h0, int w0, int64_t total) {
  const int64_t ws = (int64_t)wd * wh * ww, S = (int64_t)D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * INT_ + threadIdx.x; i < total; i += (int64_t)gridDim.x * INT_) {
    int64_t b = i / ws, v = i % ws;
    int x = (int)(v % ww), y = (int)((v / ww) % wh), z = (int)(v / ((int64_t)ww * wh));
    const float* lp = logits + (size_t)b * K * ws + v;
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) m = fmaxf(m, lp[(size_t)k * ws]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(lp[(size_t)k * ws] - m);
    const float inv = 1.f / s;
    const size_t o = ((size_t)(z + d0) * H + (y + h0)) * W + (x + w0);
    float* ap = acc + (size_t)b * K * S + o;
    for (int k = 0; k < K; ++k) ap[(size_t)k * S] += expf(lp[(size_t)k * ws] - m) * inv;
    if (counter) counter[(size_t)b * S + o] += 1.f;
  }
}

// A flip code is 3 bits: bit 0 reverses D, bit 1 H, bit 2 W.  Up to 8 codes travel packed in one kernel argument (3 bits each).
static constexpr int TTA_MAX = 8;

__device__ __forceinline__ size_t mirror_off(int code, int z, int y, int x, int wd, int wh, int ww) {
  const int fz = (code & 1) ? wd - 1 - z : z, fy = (code & 2) ? wh - 1 - y : y, fx = (code & 4) ? ww - 1 - x : x;
  return ((size_t)fz * wh + fy) * ww + fx;
}

// out[v*B + b][c][z][y][x] = img[b][c][d0 + fz][h0 + fy][w0 + fx]; one item per output element (writes coalesced; a W-reversed
// read walks the same 256-byte segments backwards)
__global__ void __launch_bounds__(INT_) k_window_gather_mirror(const float* __restrict__ img, float* __restrict__ out,
                                                               uint32_t codes, int B, int C, int wd, int wh, int ww, int D, int H,
                                                               int W, int d0, int h0, int w0, int64_t total) {
  const int64_t ws = (int64_t)wd * wh * ww, S = (int64_t)D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * INT_ + threadIdx.x; i < total; i += (int64_t)gridDim.x * INT_) {
    const int64_t p = i % ws, n = i / ws;          // n = (v*B + b)*C + c
    const int c = (int)(n % C), b = (int)((n / C) % B), v = (int)(n / ((int64_t)C * B));
    const int x = (int)(p % ww), y = (int)((p / ww) % wh), z = (int)(p / ((int64_t)ww * wh));
    const int code = (codes >> (3 * v)) & 7;
    const int fz = (code & 1) ? wd - 1 - z : z, fy = (code & 2) ? wh - 1 - y : y, fx = (code & 4) ? ww - 1 - x : x;
    out[i] = img[((size_t)b * C + c) * S + ((size_t)(fz + d0) * H + (fy + h0)) * W + (fx + w0)];
  }
}

// One item per (b, z, y, x) of the window in un-mirrored coordinates.  KT > 0: K <= KT, a variant's logits are read once and
// held in registers; KT == 0: any K, the logits are re-read (from cache) as k_softmax_accumulate does.  Both forms do the same
// float32 operations in the same order — max, expf, sum, reciprocal, product, variants summed v ascending, then one
// `acc += [w *] s` per class — so with V = 1, code 0 and no weights the result is bit-identical to k_softmax_accumulate.
template <int KT>
__global__ void __launch_bounds__(INT_) k_softmax_accumulate_tta(const float* __restrict__ logits, float* __restrict__ acc,
                                                                 float* __restrict__ wsum, const float* __restrict__ wz,
                                                                 const float* __restrict__ wy, const float* __restrict__ wx,
                                                                 uint32_t codes, int V, int B, int K, int wd, int wh, int ww,
                                                                 int D, int H, int W, int d0, int h0, int w0, int64_t total) {
  const int64_t ws = (int64_t)wd * wh * ww, S = (int64_t)D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * INT_ + threadIdx.x; i < total; i += (int64_t)gridDim.x * INT_) {
    const int64_t b = i / ws, p = i % ws;
    const int x = (int)(p % ww), y = (int)((p / ww) % wh), z = (int)(p / ((int64_t)ww * wh));
    const size_t o = ((size_t)(z + d0) * H + (y + h0)) * W + (x + w0);
    float* ap = acc + (size_t)b * K * S + o;
    const float w = wz ? (wz[z] * wy[y]) * wx[x] : 1.f;
    if constexpr (KT > 0) {
      float sk[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) sk[k] = 0.f;
      for (int v = 0; v < V; ++v) {
        const float* lp = logits + ((size_t)v * B + b) * K * ws + mirror_off((codes >> (3 * v)) & 7, z, y, x, wd, wh, ww);
        float l[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) l[k] = k < K ? lp[(size_t)k * ws] : -INFINITY;
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < KT; ++k) if (k < K) m = fmaxf(m, l[k]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) if (k < K) { l[k] = expf(l[k] - m); s += l[k]; }
        const float inv = 1.f / s;
#pragma unroll
        for (int k = 0; k < KT; ++k) if (k < K) sk[k] += l[k] * inv;
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) if (k < K) ap[(size_t)k * S] += wz ? w * sk[k] : sk[k];
    } else {
      float mv[TTA_MAX], iv[TTA_MAX];
#pragma unroll
      for (int v = 0; v < TTA_MAX; ++v) {
        mv[v] = 0.f; iv[v] = 0.f;
        if (v < V) {
          const float* lp = logits + ((size_t)v * B + b) * K * ws + mirror_off((codes >> (3 * v)) & 7, z, y, x, wd, wh, ww);
          float m = -INFINITY;
          for (int k = 0; k < K; ++k) m = fmaxf(m, lp[(size_t)k * ws]);
          float s = 0.f;
          for (int k = 0; k < K; ++k) s += expf(lp[(size_t)k * ws] - m);
          mv[v] = m; iv[v] = 1.f / s;
        }
      }
      for (int k = 0; k < K; ++k) {
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < TTA_MAX; ++v)
          if (v < V) {
            const float* lp = logits + ((size_t)v * B + b) * K * ws + mirror_off((codes >> (3 * v)) & 7, z, y, x, wd, wh, ww);
            s += expf(lp[(size_t)k * ws] - mv[v]) * iv[v];
          }
        ap[(size_t)k * S] += wz ? w * s : s;
      }
    }
    if (wsum) wsum[(size_t)b * S + o] += wz ? w * (float)V : (float)V;
  }
}

__global__ void __launch_bounds__(INT_) k_prob_finalize(float* __restrict__ acc, const float* __restrict__ counter,
                                                        int64_t* __restrict__ labels, int K, int64_t S, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * INT_ + threadIdx.x; i < total; i += (int64_t)gridDim.x * INT_) {
    int64_t b = i / S, v = i % S;
    const float c = counter ? counter[i] : 1.f;
    float* ap = acc + (size_t)b * K * S + v;
    float best = -INFINITY;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      float p = ap[(size_t)k * S] / c;
      ap[(size_t)k * S] = p;
      if (p > best) { best = p; arg = k; }      // first maximum, like torch.max
    }
    if (labels) labels[i] = arg;
  }
}

// counts[blk][c][3] (int32) for voxel blocks of `block` elements; one workgroup per block
template <typename TP, typename TT>
__global__ void __launch_bounds__(INT_) k_dice_counts(const TP* __restrict__ pred, const TT* __restrict__ target, int64_t N,
                                                      int64_t block, int C, int* __restrict__ counts) {
  CBIM_DYN_SMEM(raw);
  int* sh = (int*)raw;   // [C][3]
  for (int i = threadIdx.x; i < C * 3; i += INT_) sh[i] = 0;
  __syncthreads();
  const int64_t v0 = (int64_t)blockIdx.x * block;
  int64_t v1 = v0 + block;
  if (v1 > N) v1 = N;
  for (int64_t v = v0 + threadIdx.x; v < v1; v += INT_) {
    int p = (int)pred[v], t = (int)target[v];
    if (p >= 0 && p < C) atomicAdd(&sh[p * 3 + 1], 1);        // integer atomics: exact, order-independent
    if (t >= 0 && t < C) atomicAdd(&sh[t * 3 + 2], 1);
    if (p == t && p >= 0 && p < C) atomicAdd(&sh[p * 3], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * 3; i += INT_) counts[(size_t)blockIdx.x * C * 3 + i] = sh[i];
}

static inline int grid_for(int64_t items) {
  int64_t b = (items + INT_ - 1) / INT_;
  if (b > 256 * 16) b = 256 * 16;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace cbim

using namespace cbim;

extern "C" int cbim_softmax_accumulate(const float* logits, float* prob_sum, float* counter, int B, int K, int wd, int wh,
                                       int ww, int D, int H, int W, int d0, int h0, int w0, void* stream) {
  CBIM_CHECK(logits && prob_sum && B >= 1 && K >= 1, CBIM_EINVAL, "softmax_accumulate: bad arguments");
  CBIM_CHECK(d0 >= 0 && h0 >= 0 && w0 >= 0 && d0 + wd <= D && h0 + wh <= H && w0 + ww <= W, CBIM_EINVAL,
             "softmax_accumulate: window [%d,%d,%d]+[%d,%d,%d] outside [%d,%d,%d]", d0, h0, w0, wd, wh, ww, D, H, W);
  int64_t total = (int64_t)B * wd * wh * ww;
  CBIM_LAUNCH(k_softmax_accumulate, dim3(grid_for(total)), dim3(INT_), 0, (hipStream_t)stream, logits, prob_sum, counter, K, wd,
              wh, ww, D, H, W, d0, h0, w0, total);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

// the V flip codes of a host array, range-checked, packed 3 bits each; -1 when V or a code is out of range
static int64_t pack_codes(const int* codes, int V) {
  if (!codes || V < 1 || V > TTA_MAX) return -1;
  uint32_t packed = 0;
  for (int v = 0; v < V; ++v) {
    if (codes[v] < 0 || codes[v] > 7) return -1;
    packed |= (uint32_t)codes[v] << (3 * v);
  }
  return (int64_t)packed;
}

extern "C" int cbim_window_gather_mirror(const float* img, float* out, const int* codes, int V, int B, int C, int wd, int wh,
                                         int ww, int D, int H, int W, int d0, int h0, int w0, void* stream) {
  CBIM_CHECK(img && out && B >= 1 && C >= 1 && wd >= 1 && wh >= 1 && ww >= 1, CBIM_EINVAL, "window_gather_mirror: bad arguments");
  const int64_t packed = pack_codes(codes, V);
  CBIM_CHECK(packed >= 0, CBIM_EINVAL, "window_gather_mirror: 1 <= V <= 8 flip codes in 0..7 (V = %d)", V);
  CBIM_CHECK(d0 >= 0 && h0 >= 0 && w0 >= 0 && d0 + wd <= D && h0 + wh <= H && w0 + ww <= W, CBIM_EINVAL,
             "window_gather_mirror: window [%d,%d,%d]+[%d,%d,%d] outside [%d,%d,%d]", d0, h0, w0, wd, wh, ww, D, H, W);
  int64_t total = (int64_t)V * B * C * wd * wh * ww;
  CBIM_LAUNCH(k_window_gather_mirror, dim3(grid_for(total)), dim3(INT_), 0, (hipStream_t)stream, img, out, (uint32_t)packed, B, C,
              wd, wh, ww, D, H, W, d0, h0, w0, total);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_softmax_accumulate_tta(const float* logits, const int* codes, int V, const float* wz, const float* wy,
                                           const float* wx, float* prob_sum, float* wsum, int B, int K, int wd, int wh, int ww,
                                           int D, int H, int W, int d0, int h0, int w0, void* stream) {
  CBIM_CHECK(logits && prob_sum && B >= 1 && K >= 1 && wd >= 1 && wh >= 1 && ww >= 1, CBIM_EINVAL,
             "softmax_accumulate_tta: bad arguments");
  const int64_t packed = pack_codes(codes, V);
  CBIM_CHECK(packed >= 0, CBIM_EINVAL, "softmax_accumulate_tta: 1 <= V <= 8 flip codes in 0..7 (V = %d)", V);
  CBIM_CHECK((wz && wy && wx) || (!wz && !wy && !wx), CBIM_EINVAL,
             "softmax_accumulate_tta: the three weight vectors are given together or not at all");
  CBIM_CHECK(d0 >= 0 && h0 >= 0 && w0 >= 0 && d0 + wd <= D && h0 + wh <= H && w0 + ww <= W, CBIM_EINVAL,
             "softmax_accumulate_tta: window [%d,%d,%d]+[%d,%d,%d] outside [%d,%d,%d]", d0, h0, w0, wd, wh, ww, D, H, W);
  int64_t total = (int64_t)B * wd * wh * ww;
  const dim3 g(grid_for(total)), blk(INT_);
  hipStream_t st = (hipStream_t)stream;
  if (K <= 4)
    CBIM_LAUNCH((k_softmax_accumulate_tta<4>), g, blk, 0, st, logits, prob_sum, wsum, wz, wy, wx, (uint32_t)packed, V, B, K, wd, wh,
                ww, D, H, W, d0, h0, w0, total);
  else if (K <= 16)
    CBIM_LAUNCH((k_softmax_accumulate_tta<16>), g, blk, 0, st, logits, prob_sum, wsum, wz, wy, wx, (uint32_t)packed, V, B, K, wd, wh,
                ww, D, H, W, d0, h0, w0, total);
  else
    CBIM_LAUNCH((k_softmax_accumulate_tta<0>), g, blk, 0, st, logits, prob_sum, wsum, wz, wy, wx, (uint32_t)packed, V, B, K, wd, wh,
                ww, D, H, W, d0, h0, w0, total);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_prob_finalize(float* prob_sum, const float* counter, int64_t* labels, int B, int K, int64_t S,
                                  void* stream) {
  CBIM_CHECK(prob_sum && B >= 1 && K >= 1 && S >= 1, CBIM_EINVAL, "prob_finalize: bad arguments");
  int64_t total = (int64_t)B * S;
  CBIM_LAUNCH(k_prob_finalize, dim3(grid_for(total)), dim3(INT_), 0, (hipStream_t)stream, prob_sum, counter, labels, K, S,
              total);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

extern "C" int cbim_dice_counts(const void* pred, int pred_bytes, const void* target, int target_bytes, int64_t N,
                                int64_t block, int C, int32_t* counts, void* stream) {
  CBIM_CHECK(pred && target && counts && N >= 1 && block >= 1 && C >= 1 && C <= 1024, CBIM_EINVAL, "dice_counts: bad arguments");
  CBIM_CHECK((pred_bytes == 1 || pred_bytes == 8) && (target_bytes == 1 || target_bytes == 8), CBIM_EUNSUPPORTED,
             "dice_counts: labels must be int8 or int64");
  int nblk = (int)((N + block - 1) / block);
  size_t sh = (size_t)C * 3 * sizeof(int);
  hipStream_t st = (hipStream_t)stream;
  if (pred_bytes == 8 && target_bytes == 8)
    CBIM_LAUNCH((k_dice_counts<int64_t, int64_t>), dim3(nblk), dim3(INT_), sh, st, (const int64_t*)pred, (const int64_t*)target, N, block, C, counts);
  else if (pred_bytes == 8)
    CBIM_LAUNCH((k_dice_counts<int64_t, int8_t>), dim3(nblk), dim3(INT_), sh, st, (const int64_t*)pred, (const int8_t*)target, N, block, C, counts);
  else if (target_bytes == 8)
    CBIM_LAUNCH((k_dice_counts<int8_t, int64_t>), dim3(nblk), dim3(INT_), sh, st, (const int8_t*)pred, (const int64_t*)target, N, block, C, counts);
  else
    CBIM_LAUNCH((k_dice_counts<int8_t, int8_t>), dim3(nblk), dim3(INT_), sh, st, (const int8_t*)pred, (const int8_t*)target, N, block, C, counts);
  return CBIM_LAST_LAUNCH() == hipSuccess ? CBIM_OK : CBIM_ELAUNCH;
}

CBIM_DEFINE_WARM(inference)
