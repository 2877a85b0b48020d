// cbim_api.cpp — the process state of the C ABI (include/cbim_hip.h): version / backend / thread-local error string, and the
// kernel-selection switches of cbim_switches.h with their exported setters.  Host-only.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/cbim_hip.h"
#include "cbim_switches.h"

static thread_local char g_err[512] = "";

void cbim_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int cbim_version(void) { return 100; }
extern "C" const char* cbim_backend(void) {
#ifdef CBIM_EMU
  return "emu";
#else
  return "hip-gfx950";
#endif
}
extern "C" const char* cbim_last_error_string(void) { return g_err; }

// ---- the switches -----------------------------------------------------------------------------------------------------
namespace cbim {

namespace {
constexpr bool rows_match_ids() {
  for (int i = 0; i < SW_COUNT; ++i)
    if (SWITCHES[i].id != i) return false;
  return true;
}
static_assert(rows_match_ids(), "SWITCHES: one row per Switch id, in enum order");

struct SwitchStore {
  std::atomic<int64_t> v[SW_COUNT];
  SwitchStore() {
    for (int i = 0; i < SW_COUNT; ++i) {
      const SwitchRow& r = SWITCHES[i];
      const char* e = r.env ? getenv(r.env) : nullptr;
      v[r.id].store(e ? atoi(e) : r.def, std::memory_order_relaxed);
    }
  }
};
std::atomic<int64_t>& slot(Switch id) {
  static SwitchStore s;   // built, and the environment read, at the first use of any switch
  return s.v[id];
}
}  // namespace

int64_t sw(Switch id) { return slot(id).load(std::memory_order_relaxed); }
int64_t sw_set(Switch id, int64_t v, bool store) {
  return store ? slot(id).exchange(v, std::memory_order_relaxed) : sw(id);
}

}  // namespace cbim

using namespace cbim;

// The setters: each returns the previous value; what counts as "set" and what is stored is each one's own rule.
extern "C" int64_t cbim_conv_r32_min_voxels(int64_t v) { return sw_set(SW_CONV_R32_MIN_VOXELS, v, v >= 0); }
extern "C" int64_t cbim_up_tile_min_tiles(int64_t v) { return sw_set(SW_UP_TILE_MIN_TILES, v, v >= 0); }
extern "C" int cbim_conv_r32_tile_depth(int td) { return (int)sw_set(SW_CONV_R32_TILE_DEPTH, td, td == 4 || td == 8); }
extern "C" int cbim_wgrad_r32_waves(int w) { return (int)sw_set(SW_WGRAD_R32_WAVES, w, w == 4 || w == 8); }
extern "C" int cbim_conv_rw_enable(int on, int wide) {
  const int old_on = (int)sw_set(SW_CONV_RW, on & 1, on >= 0), old_wide = (int)sw_set(SW_CONV_RW_WIDE, wide, wide >= 0);
  return old_on | (old_wide << 1);
}
extern "C" int cbim_conv_rw48_enable(int on) { return (int)sw_set(SW_CONV_RW48, on, on >= 0); }
extern "C" int cbim_wgrad_r32_enable(int on) { return (int)sw_set(SW_WGRAD_R32, on, on >= 0); }
extern "C" int cbim_conv_pw_enable(int on) { return (int)sw_set(SW_CONV_PW, on ? 1 : 0, on >= 0); }
extern "C" int cbim_dwconv_lds_enable(int on) { return (int)sw_set(SW_DWCONV_LDS, on ? 1 : 0, on >= 0); }
extern "C" int cbim_stem_mfma_enable(int on) { return (int)sw_set(SW_STEM_MFMA, on ? 1 : 0); }
extern "C" int cbim_head_mfma_enable(int on) { return (int)sw_set(SW_HEAD_MFMA, on ? 1 : 0); }
