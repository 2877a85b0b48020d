// cbim_switches.h — every process-wide kernel-selection switch of the library, in one table.  Not part of the C ABI:
// the exported setters of include/cbim_hip.h (all defined in cbim_api.cpp) write the switches, the *_eligible / *_grid /
// launch functions of the kernel files read them with cbim::sw().  Storage is one std::atomic<int64_t> per switch with
// relaxed loads and stores: a test thread may flip a switch while autograd threads launch.
#pragma once
#include <stdint.h>

namespace cbim {

enum Switch {
  SW_CONV_R32_MIN_VOXELS,
  SW_CONV_R32_TILE_DEPTH,
  SW_CONV_RW,
  SW_CONV_RW_WIDE,
  SW_CONV_RW48,
  SW_CONV_PW,
  SW_DWCONV_LDS,
  SW_WGRAD_R32,
  SW_WGRAD_R32_C16,
  SW_WGRAD_R32_WAVES,
  SW_STEM_MFMA,
  SW_HEAD_MFMA,
  SW_UP_TILE_MIN_TILES,
  SW_COUNT
};

struct SwitchRow {
  Switch id;
  const char* name;   // the exported setter (messages); nullptr: environment only
  int64_t def;
  const char* env;    // atoi() of this variable replaces `def` when the table is first used; nullptr: none
};

constexpr SwitchRow SWITCHES[SW_COUNT] = {
    // output voxels per image from which single-chunk 3x3x3 layers run on k_conv3_r32 (the 8x8x8 threshold of k_conv_igemm); 0: always
    {SW_CONV_R32_MIN_VOXELS, "cbim_conv_r32_min_voxels", 262144, nullptr},
    // 8: one 512-thread workgroup per CU on 8x8x8 tiles; 4: two 256-thread workgroups per CU on 4x8x8 tiles — measured 5-15 %
    // slower on 32->32 @128^3 (more halo per voxel, and the MFMA phase, not the overlap, is what limits)
    {SW_CONV_R32_TILE_DEPTH, "cbim_conv_r32_tile_depth", 8, nullptr},
    // 0: every call stays on k_conv3_r32 / k_conv_igemm
    {SW_CONV_RW, "cbim_conv_rw_enable: on", 1, nullptr},
    // 0: never the wide form; 1: wherever Cout is a multiple of 64 and the grid still fills the chip; 2: wherever Cout is a multiple of 64
    {SW_CONV_RW_WIDE, "cbim_conv_rw_enable: wide", 1, nullptr},
    // 0: the 48-channel-granular layers stay on k_conv_igemm (A/B runs); 1: k_conv3_rw48 from 128 workgroups; 2: always (tests)
    {SW_CONV_RW48, "cbim_conv_rw48_enable", 1, "CBIM_CONV_RW48"},
    // 0: pointwise convolutions stay on k_conv_igemm
    {SW_CONV_PW, "cbim_conv_pw_enable", 1, nullptr},
    // 0: the streaming depthwise kernel also where the LDS-tiled one applies
    {SW_DWCONV_LDS, "cbim_dwconv_lds_enable", 1, nullptr},
    // 0: every weight gradient stays on k_conv_wgrad (tests: two-sided checks)
    {SW_WGRAD_R32, "cbim_wgrad_r32_enable", 1, nullptr},
    // 0: the layers whose channel counts are not multiples of 32 stay on k_conv_wgrad (A/B runs)
    {SW_WGRAD_R32_C16, nullptr, 1, "CBIM_WGRAD_R32_C16"},
    // waves per workgroup of k_wgrad_r32: 8 or 4
    {SW_WGRAD_R32_WAVES, "cbim_wgrad_r32_waves", 8, nullptr},
    // 0: the VALU stem kernels also where the matrix-core ones apply
    {SW_STEM_MFMA, "cbim_stem_mfma_enable", 1, nullptr},
    // 0: the VALU head backward also where the matrix-core kernel applies
    {SW_HEAD_MFMA, "cbim_head_mfma_enable", 1, nullptr},
    // fewest fine tiles per image the tiled up-sampling kernels take; 0: any
    {SW_UP_TILE_MIN_TILES, "cbim_up_tile_min_tiles", 512, nullptr},
};

// current value (relaxed load).  One decision reads a switch once.
int64_t sw(Switch id);
// returns the current value and, when `store` holds, replaces it with v (relaxed exchange)
int64_t sw_set(Switch id, int64_t v, bool store = true);

}  // namespace cbim
