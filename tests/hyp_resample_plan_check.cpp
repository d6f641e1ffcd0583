// Sanitizer build of the host side of the hypothesis bank's resampling (slam-duckietown_amd/csrc/ekf_host_plan.h:
// plan_hyp_resample, hyp_plan_chunk, hyp_copy_groups, hyp_resample_ints; ekf_device.h: HypWeighOut):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DEKF_HOST_ONLY
//       -I slam-duckietown_amd/csrc -I include tests/hyp_resample_plan_check.cpp -o hyp_resample_plan_check
// Every refusal (u, split, z), keep = 1 - s^2, the chunks of the one-workgroup kernels at K = 1, 65, 1024, 1025, 65536, the
// column groups at ldx = 64, 320, 512, 4160 with the bounds a workgroup's lanes keep, and draws allocated to exactly count x 3
// doubles, so that a read beyond them is a sanitizer report; any report or failed check ends the run with a non-zero status.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "plan_check.h"

using namespace ekf;

static HypBank make_bank(int count, int ldx) {
  HypBank hy;
  hy.n = std::min(ldx, 43);
  hy.ld = hy.ldx = ldx;
  hy.count = count;
  return hy;
}

static bool says(const char* why, const char* part) { return why && std::strstr(why, part); }

int main() {
  CHECK(sizeof(HypWeighOut) == 64 && sizeof(HypWeighOut) % 16 == 0, "HypWeighOut is %zu bytes", sizeof(HypWeighOut));
  CHECK(HYP_PLAN_THREADS == 1024 && HYP_PLAN_THREADS % 64 == 0 && HYP_PLAN_THREADS / 64 <= 16, "the scans keep 16 wave totals");
  CHECK(HYP_COPY_COLS == 2 * HYP_THREADS, "a lane moves two columns");
  const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
  // ---- the shapes ----
  for (int K : {1, 65, 1024, 1025, 65535, 65536}) {
    const int chunk = hyp_plan_chunk(K);
    CHECK(chunk >= 1 && chunk <= 64 && (long)chunk * HYP_PLAN_THREADS >= K && (long)(chunk - 1) * HYP_PLAN_THREADS < K, "chunk %d for K = %d", chunk, K);
    // every record belongs to exactly one thread: thread t walks [min(K, t chunk), min(K, t chunk + chunk))
    long covered = 0;
    for (int t = 0; t < HYP_PLAN_THREADS; ++t) {
      const int k0 = std::min(K, t * chunk), k1 = std::min(K, k0 + chunk);
      CHECK(k0 == covered && k1 >= k0, "thread %d starts at %d, %ld covered", t, k0, covered);
      covered = k1;
    }
    CHECK(covered == K, "K = %d: %ld records covered", K, covered);
    CHECK(hyp_resample_ints(K) == 3 * (size_t)K, "scratch ints");
    CHECK(K <= HYP_COUNT_MAX && (long)K <= 2147483647L, "K = %d is a grid.x", K);
  }
  CHECK(hyp_plan_chunk(1) == 1 && hyp_plan_chunk(1024) == 1 && hyp_plan_chunk(1025) == 2 && hyp_plan_chunk(65536) == 64, "chunks");
  for (int ldx : {64, 320, 512, 4160}) {
    const int g = hyp_copy_groups(ldx);
    CHECK(g >= 1 && g <= 65535 && g * HYP_COPY_COLS >= ldx && (g - 1) * HYP_COPY_COLS < ldx, "groups %d for ldx %d", g, ldx);
    // the lanes of the last group: column c = 2 (group * HYP_THREADS + lane) moves c and c + 1 where c < ldx
    for (int lane = 0; lane < HYP_THREADS; ++lane) {
      const int c = 2 * ((g - 1) * HYP_THREADS + lane);
      if (c < ldx) CHECK(c + 1 < ldx && c % 2 == 0, "lane %d of the last group reaches column %d of %d", lane, c + 1, ldx);
    }
  }
  CHECK(hyp_copy_groups(64) == 1 && hyp_copy_groups(320) == 1 && hyp_copy_groups(512) == 1 && hyp_copy_groups(4160) == 9, "column groups");
  // ---- the arguments ----
  for (int K : {1, 65, 65536}) {
    const HypBank hy = make_bank(K, 64);
    std::vector<double> z(3 * (size_t)K, 0.25);                            // exactly count x 3
    HypResamplePlan rp;
    CHECK(plan_hyp_resample(&hy, 0.0, 0.0, nullptr, rp) == nullptr && !rp.split && rp.keep == 1.0 && rp.u == 0.0, "copies only");
    CHECK(rp.chunk == hyp_plan_chunk(K) && rp.groups == 1, "K = %d: chunk %d groups %d", K, rp.chunk, rp.groups);
    CHECK(plan_hyp_resample(&hy, 1.0 - std::ldexp(1.0, -53), 0.0, nullptr, rp) == nullptr, "the largest u");
    CHECK(plan_hyp_resample(&hy, 0.5, 0.5, z.data(), rp) == nullptr && rp.split && rp.s == 0.5 && rp.keep == 0.75, "a split: keep %g", rp.keep);
    CHECK(plan_hyp_resample(&hy, 0.5, 0.6, z.data(), rp) == nullptr && rp.keep == 1.0 - 0.6 * 0.6, "keep is 1 - s s");
    for (double u : {1.0, -1e-9, 2.0, nan, inf, -inf}) CHECK(says(plan_hyp_resample(&hy, u, 0.0, nullptr, rp), "u must be"), "u = %g", u);
    for (double s : {1.0, -0.1, 1.5, nan, inf}) CHECK(says(plan_hyp_resample(&hy, 0.5, s, z.data(), rp), "split must be"), "split = %g", s);
    CHECK(says(plan_hyp_resample(&hy, 0.5, 0.5, nullptr, rp), "needs z"), "a split without draws");
    CHECK(says(plan_hyp_resample(&hy, 0.5, 0.0, z.data(), rp), "split == 0"), "draws without a split");
    z[3 * (size_t)K - 1] = nan;                                           // the last entry is read ...
    CHECK(says(plan_hyp_resample(&hy, 0.5, 0.5, z.data(), rp), "non-finite z"), "a NaN draw");
    z[3 * (size_t)K - 1] = inf;
    CHECK(says(plan_hyp_resample(&hy, 0.5, 0.5, z.data(), rp), "non-finite z"), "an infinite draw");
    z[3 * (size_t)K - 1] = 0.0;
    z[0] = -inf;                                                          // ... and the first
    CHECK(says(plan_hyp_resample(&hy, 0.5, 0.5, z.data(), rp), "non-finite z"), "the first draw");
    // a refusal names u before split before z (the header's order)
    CHECK(says(plan_hyp_resample(&hy, nan, 2.0, nullptr, rp), "u must be") && says(plan_hyp_resample(&hy, 0.5, 2.0, nullptr, rp), "split must be"),
          "the order of the refusals");
  }
  for (int ldx : {64, 320, 4160}) {
    const HypBank hy = make_bank(65, ldx);
    HypResamplePlan rp;
    CHECK(plan_hyp_resample(&hy, 0.25, 0.0, nullptr, rp) == nullptr && rp.groups == hyp_copy_groups(ldx), "ldx = %d", ldx);
  }
  {
    HypResamplePlan rp;
    const HypBank odd = make_bank(4, 63), none = make_bank(0, 64);
    CHECK(says(plan_hyp_resample(&odd, 0.5, 0.0, nullptr, rp), "shape") && says(plan_hyp_resample(&none, 0.5, 0.0, nullptr, rp), "shape"),
          "a bank the kernels' 16-byte lanes cannot walk");
  }
  std::printf("%ld checks passed\n", checks);
  return 0;
}
