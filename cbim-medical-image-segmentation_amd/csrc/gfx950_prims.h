// gfx950_prims.h — the gfx950 (MI355X / CDNA4) hardware primitives of the kernel files, each defined ONCE: the hardware arm and
// the CBIM_EMU arm (tests/emu: host-side executor of the CPU test-suite) side by side, and each hazard explained where the
// primitive is defined.  A kernel file takes its primitives from here and declares none of its own.
#pragma once
#include "cbim_common.h"

#ifdef CBIM_EMU
#define CBIM_DYN_SMEM(name) unsigned char* name = cbim_emu::dyn_smem()
#define CBIM_SCHED_FENCE() ((void)0)
#else
// the workgroup's dynamic LDS as a 16-byte aligned byte array
#define CBIM_DYN_SMEM(name) extern __shared__ __attribute__((aligned(16))) unsigned char name[]
// nothing is scheduled across it: pins "issue these LDS reads, THEN run those MFMAs" in a software pipeline
#define CBIM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

namespace cbim {

// ---- LDS-DMA --------------------------------------------------------------------------------------------------------------
// One 1 KiB piece: lane l copies 16 bytes from its own global address to (wave-uniform LDS base) + 16 l — no registers, no
// vector ALU.  Two forms: from a per-lane global pointer, and through a buffer descriptor.
//   * Issued through inline asm ON PURPOSE: with the builtin the compiler knows an LDS-DMA is in flight, treats the LGKM
//     counter as out-of-order and turns every `s_waitcnt lgkmcnt(n)` of a fragment pipeline into lgkmcnt(0) — each MFMA pair
//     then waits a full LDS round trip.  The compiler therefore does NOT know the DMA is in flight: its completion is the
//     caller's explicit wait_vm<N>() + barrier.
//   * M0 (the LDS base of the instruction) is saved and restored INSIDE the statement: no reserved register in the clobber
//     list (clang: "may lead to undefined behaviour"), nothing about M0 is hidden from the compiler.
__device__ __forceinline__ void lds_dma16(const unsigned char* gsrc, unsigned char* lds_wave_base) {
#ifdef CBIM_EMU
  emu_global_load_lds16(gsrc, lds_wave_base);
#else
  unsigned a = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds_wave_base;
  a = __builtin_amdgcn_readfirstlane(a);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(a), "v"(gsrc) : "memory");
#endif
}
// the same piece through a buffer descriptor, to LDS byte lds_base + off (lds_base = the 32-bit LDS address of smem): lane l
// copies the 16 bytes at base + soff + voff, ZEROS when soff + voff + 16 > nrec — zero padding is the range check (a lane
// outside the tensor carries voff = 0x80000000, a plane outside the tensor nrec = 0), the tile / plane origin travels in the
// scalar offset
__device__ __forceinline__ void lds_dma16_buf(unsigned voff, unsigned long long base, unsigned nrec, unsigned soff,
                                              unsigned char* smem, unsigned lds_base, unsigned off) {
#ifdef CBIM_EMU
  (void)lds_base;
  emu_buffer_load_lds16((const unsigned char*)base, nrec, voff, soff, smem + off);
#else
  (void)smem;
  i32x4 rs = {(int)(unsigned)base, (int)((unsigned)(base >> 32) & 0xffffu), (int)nrec, 0x00020000};
  rs.x = __builtin_amdgcn_readfirstlane(rs.x); rs.y = __builtin_amdgcn_readfirstlane(rs.y);
  rs.z = __builtin_amdgcn_readfirstlane(rs.z);
  const unsigned a = __builtin_amdgcn_readfirstlane(lds_base + off), so = __builtin_amdgcn_readfirstlane(soff);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(a), "v"(voff), "s"(rs), "s"(so) : "memory");
#endif
}

// at most N vector-memory operations of this wave still in flight (they return in order: everything older than the last N
// has landed — the LDS-DMA pieces above included, which the compiler's own waits do not cover)
template <int N>
__device__ __forceinline__ void wait_vm() {
#ifndef CBIM_EMU
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}
__device__ __forceinline__ void wait_lgkm0() {
#ifndef CBIM_EMU
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}

// ---- integer helpers ------------------------------------------------------------------------------------------------------
// 24-bit multiply / multiply-add (full rate; the generic 32-bit multiply is quarter rate): both factors below 2^24
__device__ __forceinline__ unsigned umul24(unsigned a, unsigned b) {
#ifdef CBIM_EMU
  return a * b;
#else
  return __umul24(a, b);
#endif
}
__device__ __forceinline__ unsigned umad24(unsigned a, unsigned b, unsigned c) { return umul24(a, b) + c; }
// optimisation barrier on a VGPR: makes a loop-invariant value look freshly computed, so it (and what is derived from it)
// stays inside the loop instead of occupying registers across it
__device__ __forceinline__ unsigned launder(unsigned v) {
#ifndef CBIM_EMU
  asm volatile("" : "+v"(v));
#endif
  return v;
}
// a value the caller knows to be wave-uniform, moved to a scalar register
__device__ __forceinline__ int uniform(int v) {
#ifdef CBIM_EMU
  return v;
#else
  return __builtin_amdgcn_readfirstlane(v);
#endif
}

// ---- exchanges inside one wave --------------------------------------------------------------------------------------------
// rendez-vous for LDS data exchanged between lanes of ONE wave (LDS executes a wave's instructions in order; only the
// compiler — and the host-side executor, whose lanes are fibers — must not reorder across it)
__device__ __forceinline__ void wave_sync() {
#ifdef CBIM_EMU
  int z = 0;
  (void)cbim_emu::wave_exchange(&z, sizeof(z));
#else
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}
// ordered counting inside one wave (the ballot itself: wave_ballot of atomics_compat.h).  ballot_rank: how many lanes BELOW
// `lane` have their bit set — with the ballot of a predicate, the lane's rank among the lanes where it holds, in lane order.
__device__ __forceinline__ int ballot_rank(unsigned long long ballot, int lane) {
  return __builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}
// inclusive prefix sum over the 64 lanes, in lane order (six ds_bpermute steps: for latency-bound selects, not for hot loops)
__device__ __forceinline__ long long wave_scan_incl(long long v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl(v, (lane - d) & 63, 64);
    if (lane >= d) v += o;
  }
  return v;
}
// 4 consecutive-voxel bf16 of one channel via the LDS transpose read ds_read_b64_tr_b16 (per-lane address of 4 bf16)
__device__ __forceinline__ u32x2 lds_tr16_b64(const unsigned char* p) {
#ifdef CBIM_EMU
  unsigned short o[4];
  emu_ds_read_tr16_b64(p, o);
  u32x2 r;
  r.x = (unsigned)o[0] | ((unsigned)o[1] << 16);
  r.y = (unsigned)o[2] | ((unsigned)o[3] << 16);
  return r;
#else
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
  return __builtin_bit_cast(u32x2, v);
#endif
}
// partner value of the butterfly step MSK of an all-reduce over the wave.  Steps 1 and 2 are quad permutes, steps 4 and 8 the
// half-row / row mirrors of the data-parallel-primitive path (vector-ALU rate): after steps 1, 2 the four lanes of a quad
// hold the same value, so the mirror partner (other quad, any lane) is as good as lane ^ 4 — bit-identical to the xor
// butterfly, PROVIDED the steps run in the order 1, 2, 4, 8.  Only steps >= 16 cross 16-lane rows and go through the LDS
// crossbar: __shfl_xor is a ds_bpermute, an LDS round trip of ~100 cycles, DPP is not (all five steps as ds_bpermute were 85
// LDS round trips per tile in the multi-chunk convolution epilogues, twelve dependent ones per map row 10 us per chunk).
template <int MSK>
__device__ __forceinline__ float dpp_bfly(float v) {
#ifdef CBIM_EMU
  return __shfl_xor(v, MSK, 64);
#else
  if (MSK >= 16) return __shfl_xor(v, MSK, 64);
  constexpr int ctrl = MSK == 1 ? 0xB1 : MSK == 2 ? 0x4E : MSK == 4 ? 0x141 : 0x140;   // quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
#endif
}
// exchange between 16-lane rows: a's odd rows (lanes 16..31, 48..63) <-> b's even rows (lanes 0..15, 32..47)
// (v_permlane16_swap_b32)
__device__ __forceinline__ void swap16(float& a, float& b) {
#ifdef CBIM_EMU
  struct P { float a, b; } mine = {a, b};
  const P* buf = (const P*)cbim_emu::wave_exchange(&mine, sizeof(P));
  const int l = CBIM_EMU_LANE_ID();
  if (l & 16) a = buf[l - 16].b;
  else b = buf[l + 16].a;
#else
  u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r.x);
  b = __uint_as_float(r.y);
#endif
}

// XOR key of the 16-byte slot inside the 64-byte LDS row of halo position (hd, hh, hw), by the row's h coordinate.  A
// ds_read_b128 lane group of the B-fragment read covers the two h rows of the wave's patch and two k-groups: keys 0 / 2 on
// alternating rows give it 16 distinct cells of the 256-byte bank window (key hh & 3, right for the 4-row patches of
// conv_igemm.hip, measured 37 % conflict cycles on 2-row patches).  The four 16-lane groups of a transposed read sit on four
// consecutive h rows (640 / 512 bytes apart = 128 / 0 modulo the bank window): the same key spreads them over all banks.
__device__ __forceinline__ unsigned halo_swz(unsigned hh) { return (hh & 1u) << 1; }

}  // namespace cbim
