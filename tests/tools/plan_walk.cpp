// Host-only sanitizer walk of the workspace plan (csrc/mgs_plan.hip): every entry point over the grid of tests/plan_cases.py,
// plus shapes whose products P x T, V x P x F and 3 x M x G pass 2^31.  No device, no Python:
// (-Xarch_host keeps the sanitizers to the host pass; the link line's flag only selects their runtimes, and hipcc may remark
//  that the device side ignores it)
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=undefined,address -Xarch_host -fno-sanitize-recover=all \
//     -c manigaussian_amd/csrc/mgs_plan.hip -o mgs_plan.o
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=undefined,address -Xarch_host -fno-sanitize-recover=all \
//     -c tests/tools/plan_walk.cpp -o plan_walk.o
//   hipcc -fsanitize=undefined,address mgs_plan.o plan_walk.o -o plan_walk && ./plan_walk
// Exit status 1 if a shape of the grid is refused; the larger shapes may be (their refusals are counted and printed).
#include <stdio.h>

#include "../../include/mgsplat.h"

namespace mgs { void set_error(const char*, ...) {} }  // (the library's lives in mgs_api.hip, beside the HIP calls)

int main() {
  const int Ps[] = {1, 1000, 16384, 100000, 500000, 2000000, 134217727}, WH[][2] = {{16, 16}, {128, 128}, {256, 256}, {1024, 1024},
                   {1040, 1024}, {1920, 1080}, {32768, 32768}}, Fs[] = {0, 3, 32, 64}, Vs[] = {0, 1, 4, 16};
  const int64_t budgets[] = {0, (int64_t)1 << 30, (int64_t)9 << 30};
  long n = 0, bad = 0, grid_bad = 0;
  for (int P : Ps) for (auto& wh : WH) for (int F : Fs) for (int V : Vs) for (int S : {0, V}) for (int M : {0, 4, 16}) {
    const MgsPlanShape s{P, M, F, wh[0], wh[1], V, S, S > 0};
    MgsArenaPlan a; MgsGradientPlan g; int64_t cap, pool;
    const long before = bad;
    for (int64_t b : budgets) bad += mgs_plan_arena(&s, b, &a) != MGS_OK;
    bad += mgs_plan_gradients(&s, &g) != MGS_OK;
    for (int64_t R : {(int64_t)-1, (int64_t)0, a.worst_capacity, (int64_t)1 << 40}) {
      bad += mgs_plan_capacity(&s, MGS_SIZE_COUNT, R, 0, 1.0, 1.0, &cap, &pool) != MGS_OK;
      n += mgs_plan_binning_bytes(&s, cap, 0, 1) != 0;
      bad += R >= 0 && mgs_plan_capacity(&s, MGS_SIZE_HEADROOM, R, R / 64, 1.5, 2.0, &cap, &pool) != MGS_OK;
      n += mgs_plan_binning_bytes(&s, cap, pool, 0) != 0;
      MgsOptions o{};
      o.seg = 2048; o.bin_mode = 2;
      bad += mgs_plan_options(&s, R, &o) != MGS_OK;
    }
    if (P <= 2000000 && wh[0] <= 1920) grid_bad += bad - before;
  }
  printf("plan_walk: %ld binning sizes, %ld refusals, %ld of them inside the grid\n", n, bad, grid_bad);
  return grid_bad != 0;
}
