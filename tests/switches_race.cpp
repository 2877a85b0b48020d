// Stand-alone ThreadSanitizer check of the switch table (csrc/cbim_switches.h, csrc/cbim_api.cpp): two threads hammer the
// exported setters while two threads read cbim::sw(), as the test suite and the autograd threads of a DDP run do.  Built by
// tests/test_switches_race.py from cbim_api.cpp and this file alone with -fsanitize=thread; host code only, no GPU.
#include <stdio.h>

#include <atomic>
#include <thread>

#include "../include/cbim_hip.h"
#include "../cbim-medical-image-segmentation_amd/csrc/cbim_switches.h"

using namespace cbim;

static constexpr int ROUNDS = 50000;   // per writer: a fraction of a second under the sanitizer
static std::atomic<int> g_writers{2};

static void writer(int k) {
  for (int i = k; i < ROUNDS; ++i) {
    cbim_conv_r32_min_voxels(i & 1 ? 0 : 262144);
    cbim_conv_r32_tile_depth(i & 1 ? 4 : 8);
    cbim_conv_rw_enable(i & 1, i & 2 ? -1 : 1);
    cbim_conv_rw48_enable(i % 3);
    cbim_conv_pw_enable(i & 1);
    cbim_dwconv_lds_enable(i & 1);
    cbim_wgrad_r32_enable(i & 1);
    cbim_wgrad_r32_waves(i & 1 ? 4 : 8);
    cbim_stem_mfma_enable(i & 1);
    cbim_head_mfma_enable(i & 1);
    cbim_up_tile_min_tiles(i & 1 ? 0 : 512);
  }
  g_writers.fetch_sub(1);
}

static void reader(long long* bad) {
  do {
    for (int id = 0; id < SW_COUNT; ++id) {
      const int64_t v = sw((Switch)id);
      if (v < 0 || v > 262144) ++*bad;   // only values some writer stored, or a default, may ever be seen
    }
  } while (g_writers.load(std::memory_order_relaxed) > 0);
}

int main() {
  long long bad[2] = {0, 0};
  std::thread t[4] = {std::thread(writer, 0), std::thread(writer, 1), std::thread(reader, &bad[0]), std::thread(reader, &bad[1])};
  for (auto& th : t) th.join();
  if (bad[0] || bad[1]) {
    fprintf(stderr, "a reader saw a value nobody stored (%lld times)\n", bad[0] + bad[1]);
    return 1;
  }
  puts("switches_race: clean");
  return 0;
}
