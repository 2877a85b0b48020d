// radix_select.h — what the exact, sort-free order statistics of a float32 array share (predict_kernels.hip: k_os_hist /
// k_os_pick, the intensity percentiles; topk_kernels.hip: the threshold of the top-k cross entropy): the order-preserving
// integer image of the float bits and the step that narrows a rank to one digit of a 256-bin histogram.  Four such steps,
// one per 8 bits of the key from the top, fix the key of the element at a given ascending rank.
#pragma once
#include "cbim_common.h"

namespace cbim {

// ascending unsigned keys <=> ascending floats (-0 sorts right below +0)
__device__ __forceinline__ unsigned os_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float os_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// The digit whose bin holds ascending rank `rem` among the keys counted in hist[256] (the last bin if the counts end
// before it); `rem` becomes the rank inside that bin.  The cumulative counts never decrease, so the bins at or below
// `rem` are a prefix: counting them needs no early exit, and the 255 loads do not wait for one another.
__device__ __forceinline__ unsigned os_narrow(const unsigned* hist, unsigned& rem) {
  unsigned d = 0u, below = 0u, cum = 0u;
#pragma unroll 15
  for (int i = 0; i < 255; ++i) {
    cum += hist[i];
    const bool past = cum <= rem;
    d += past ? 1u : 0u;
    below = past ? cum : below;
  }
  rem -= below;
  return d;
}

}  // namespace cbim
