// atomics_compat.h — the integer atomics, the agent-scope load and the wave ballot that components_kernels.hip uses, under one
// spelling for both builds.  On the device they are the HIP intrinsics; under CBIM_EMU (the host-side executor of the CPU
// test-suite, tests/emu/hip_emu.h, which has atomicAdd and a 32-bit atomicMax only) they are built on __atomic_* and on the
// executor's wave rendez-vous, in the style of the shims there.
#pragma once
#include "cbim_common.h"

#ifdef CBIM_EMU
inline int atomicMin(int* p, int v) {
  int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
#endif

namespace cbim {

// relaxed load that other workgroups' atomics of the same launch are visible to (device: bypasses the CU's L1)
__device__ __forceinline__ int load_agent(const int* p) {
#ifdef CBIM_EMU
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// bit l = predicate of lane l of the wave; every lane of the wave must call it
__device__ __forceinline__ unsigned long long wave_ballot(int pred) {
#ifdef CBIM_EMU
  const int mine = pred != 0;
  const unsigned char* buf = cbim_emu::wave_exchange(&mine, sizeof(int));
  unsigned long long r = 0;
  for (int i = 0; i < 64; ++i) { int v; memcpy(&v, buf + (size_t)i * sizeof(int), sizeof(int)); r |= (unsigned long long)(v != 0) << i; }
  return r;
#else
  return __ballot(pred);
#endif
}

}  // namespace cbim
