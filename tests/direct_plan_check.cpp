// Sanitizer build of plan_direct and pack_direct (slam-duckietown_amd/csrc/ekf_host_plan.h), the host-side validation, row
// plan and launch table of ekf_update_direct:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DEKF_HOST_ONLY
//       -I slam-duckietown_amd/csrc -I include tests/direct_plan_check.cpp -o direct_plan_check
// Every refusal the header lists, the row plan of accepted calls, and randomised calls at the limits (stride = EKF_MMAX, a
// pose fix plus 15 landmarks = 33 rows); behind every accepted plan the table pack_direct makes of it, into vectors it sizes
// itself (a write beyond them is a sanitizer report), against a second, naive indexing; any sanitizer report or failed check
// ends the run with a non-zero status.
// tests/test_direct_cpu.py builds and runs it (CPU only).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "plan_check.h"

using namespace ekf;

struct Call {
  int b0 = 0, count = 2, stride = 4;
  std::vector<int> target{-1, 2, 5, 0, -2, 1, 0, 0}, m{3, 2};
  std::vector<double> z, R, gate;
  bool null_target = false, null_z = false, null_R = false, null_m = false;
  Call() : z(2 * 4 * 3, 0.5), R(2 * 4 * 9, 0.0) {
    for (int f = 0; f < 8; ++f) {
      R[9 * f + 0] = 0.01;
      R[9 * f + 4] = 0.02;
      R[9 * f + 8] = 0.001;
      R[9 * f + 1] = 0.002;
      R[9 * f + 3] = 1e300;                                  // below the diagonal: never read
    }
  }
  const char* plan(const HostPlan& h, DirectPlan& dp) const {
    return plan_direct(&h, b0, count, null_target ? nullptr : target.data(), null_z ? nullptr : z.data(),
                       null_R ? nullptr : R.data(), null_m ? nullptr : m.data(), stride, gate.empty() ? nullptr : gate.data(), dp);
  }
};

// The table of an accepted call: sizes as the launch's buffer is laid out ({ints | doubles | 2 B results}), every trajectory
// of the bank its own bound, those outside the range no row, those inside their plan's rows -- state indices inside the
// state, D within the launch's row cap -- and every z, R and gate where a naive indexing of DIRECT_INTS / DIRECT_DBLS puts it.
static void check_pack(const HostPlan& h, const Call& c, const DirectPlan& dp) {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<int> ints;
  std::vector<double> dbls;
  pack_direct(&h, dp, c.b0, c.count, c.z.data(), c.R.data(), c.m.data(), c.stride, c.gate.empty() ? nullptr : c.gate.data(), ints, dbls);
  const size_t B = (size_t)h.batch;
  CHECK(ints.size() == B * (2 + 2 * 36) && dbls.size() == B * (EKF_MMAX * 12 + 2), "sizes %zu %zu", ints.size(), dbls.size());
  const FrontTable tab = direct_table();
  CHECK(tab.ints * B == ints.size() && tab.dbls * B == dbls.size() && tab.int_words(B) * 2 >= ints.size() && tab.int_words(B) * 2 <= ints.size() + 1 &&
            tab.words(B) == (ints.size() + 1) / 2 + dbls.size() + 2 * B, "table of %zu words", tab.words(B));
  const int cap = front_rows_cap(dp.kpad, DIRECT_ROWS);
  CHECK(cap == (dp.kpad <= 4 ? 4 : dp.kpad <= 8 ? 8 : dp.kpad <= 16 ? 16 : 36) && cap >= dp.kpad, "cap %d for kpad %d", cap, dp.kpad);
  for (int b = 0; b < h.batch; ++b) {
    const int* pi = ints.data() + (size_t)b * 74;
    const double* pd = dbls.data() + (size_t)b * 194;
    const int bi = b - c.b0;
    const bool inside = bi >= 0 && bi < c.count;
    CHECK(pi[1] == (h.opt_active_bound ? std::min(h.neff[b], h.n[b]) : h.n[b]), "bound of %d: %d", b, pi[1]);
    CHECK(pi[0] == (inside ? dp.D[bi] : 0) && pi[0] <= cap, "D of %d: %d", b, pi[0]);
    for (int k = 0; k < 36; ++k) {
      const int s = pi[2 + k], src = pi[2 + 36 + k];
      if (k >= pi[0]) { CHECK(s == -1 && src == 0, "pad row %d of %d: %d %d", k, b, s, src); continue; }
      CHECK(s >= 0 && s < h.n[b], "row %d of %d -> %d", k, b, s);
      const int j = src >> 2, a = src & 3;
      const size_t f = (size_t)bi * c.stride + j;
      CHECK(j < c.m[bi] && a < direct_rows(c.target[f]), "src %d", src);
      CHECK(s == (c.target[f] < 0 ? a : 3 + 2 * c.target[f] + a), "row %d of %d: state index %d", k, b, s);
      CHECK(pd[3 * j + a] == c.z[3 * f + a], "z of row %d", k);
      for (int q = a; q < direct_rows(c.target[f]); ++q) CHECK(pd[3 * EKF_MMAX + 9 * j + 3 * a + q] == c.R[9 * f + 3 * a + q], "R of row %d", k);
    }
    CHECK(pd[192] == (inside ? (c.gate.empty() ? inf : c.gate[bi]) : 0.0) && pd[193] == 0.0, "gate of %d: %g", b, pd[192]);
    if (!inside)
      for (int e = 0; e < 194; ++e) CHECK(pd[e] == 0.0, "doubles of %d outside the range", b);
  }
}

// a call of one trajectory with D rows: a pose fix where D is odd, landmarks `first`, first + 1, ... for the rest
static Call rows_call(int D, int stride, int b0, int first) {
  Call c;
  c.b0 = b0, c.count = 1, c.stride = stride;
  c.m = {D / 2};
  c.target.assign(stride, 0);
  c.z.assign((size_t)stride * 3, 0.0);
  c.R.assign((size_t)stride * 9, 0.0);
  for (int j = 0; j < stride; ++j) {
    c.target[j] = (D & 1) && j == 0 ? EKF_DIRECT_POSE : first + j;
    for (int a = 0; a < 3; ++a) {
      c.z[3 * j + a] = 100.0 * j + a + 0.5;
      for (int q = 0; q < 3; ++q) c.R[9 * j + 3 * a + q] = a == q ? 0.01 * (j + 1) : q > a ? 0.001 * (a + q) : 1e300;
    }
  }
  return c;
}

int main() {
  HostPlan h;
  h.batch = 3;
  h.n = {3 + 2 * 40, 3 + 2 * 10, 3 + 2 * 20};
  h.neff = {3 + 2 * 30, 3 + 2 * 10, 3};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  DirectPlan dp;
  {
    Call c;
    CHECK(c.plan(h, dp) == nullptr, "the good call");
    CHECK(dp.kpad == 8 && dp.D[0] == 7 && dp.D[1] == 4, "%d %d %d", dp.kpad, dp.D[0], dp.D[1]);
    const int want0[7] = {0, 1, 2, 7, 8, 13, 14}, src0[7] = {0, 1, 2, 4, 5, 8, 9}, want1[4] = {0, 1, 5, 6};
    for (int k = 0; k < 7; ++k) CHECK(dp.s[k] == want0[k] && dp.src[k] == src0[k], "row %d", k);
    for (int k = 0; k < 4; ++k) CHECK(dp.s[DIRECT_ROWS + k] == want1[k], "row %d", k);
    for (int k = 7; k < DIRECT_ROWS; ++k) CHECK(dp.s[k] == -1, "pad %d", k);
    check_pack(h, c, dp);
    c.gate = {inf, 11.3};
    CHECK(c.plan(h, dp) == nullptr, "gates");
    check_pack(h, c, dp);
    c.m = {0, 0};
    CHECK(c.plan(h, dp) == nullptr && dp.kpad == 0, "nothing to do");
    check_pack(h, c, dp);
  }
  auto refused = [&](const Call& c, const char* what) {
    const char* why = c.plan(h, dp);
    CHECK(why != nullptr, "%s was accepted", what);
  };
  { Call c; c.b0 = 2; refused(c, "range past the bank"); }
  { Call c; c.b0 = -1; refused(c, "negative b0"); }
  { Call c; c.count = 0; refused(c, "count 0"); }
  { Call c; c.stride = 0; refused(c, "stride 0"); }
  { Call c; c.stride = EKF_MMAX + 1; refused(c, "stride 17"); }
  { Call c; c.m[0] = 5; refused(c, "m above stride"); }
  { Call c; c.m[1] = -1; refused(c, "negative m"); }
  { Call c; c.target[5] = 10; refused(c, "landmark outside trajectory 1's map"); }
  { Call c; c.target[2] = -3; refused(c, "target -3"); }
  { Call c; c.target[2] = 2; refused(c, "landmark twice"); }
  { Call c; c.target[2] = -2; refused(c, "pose and position"); }
  { Call c; c.target[2] = -1; refused(c, "pose twice"); }
  { Call c; c.z[3 * 5 + 1] = nan; refused(c, "NaN z"); }
  { Call c; c.z[2] = inf; refused(c, "infinite theta"); }
  { Call c; c.R[2] = inf; refused(c, "infinite R"); }
  { Call c; c.R[9 * 1 + 1] = 0.02; refused(c, "2 x 2 R not positive definite"); }
  { Call c; c.R[0] = 0.0; refused(c, "zero variance"); }
  { Call c; c.R[2] = 0.2; refused(c, "3 x 3 R not positive definite"); }
  { Call c; c.gate = {nan, 1.0}; refused(c, "NaN gate"); }
  { Call c; c.gate = {1.0, 0.0}; refused(c, "zero gate"); }
  { Call c; c.gate = {-inf, 1.0}; refused(c, "negative gate"); }
  { Call c; c.null_target = true; refused(c, "NULL target"); }
  { Call c; c.null_z = true; refused(c, "NULL z"); }
  { Call c; c.null_R = true; refused(c, "NULL R"); }
  { Call c; c.null_m = true; refused(c, "NULL m"); }
  // the third z entry and R's third row / column of a 2-row fix are ignored
  { Call c; c.z[3 * 1 + 2] = nan; c.R[9 * 1 + 8] = nan; c.R[9 * 1 + 2] = nan; CHECK(c.plan(h, dp) == nullptr, "ignored entries"); check_pack(h, c, dp); }
  // D at 0 and at each edge of a row cap (4 | 5, 8 | 9, 16 | 17, 32 fixes' worth at EKF_MMAX fixes, the full 33), strides at and
  // far above the count: a bank of one, and the middle trajectory of three with the active bound off and on
  {
    HostPlan one;
    one.batch = 1;
    one.n = {3 + 2 * 40};
    one.neff = {3 + 2 * 25};
    for (int D : {0, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33})
      for (int stride : {std::max(1, D / 2), EKF_MMAX}) {
        Call c = rows_call(D, stride, 0, 7);
        CHECK(c.plan(one, dp) == nullptr && dp.D[0] == D && dp.kpad == ((D + 3) & ~3), "D = %d: %d, kpad %d", D, dp.D[0], dp.kpad);
        check_pack(one, c, dp);
        if (D > 20) continue;                                // (trajectory 1 of `h` has 10 landmarks)
        c = rows_call(D, stride, 1, 0);
        c.gate = {7.5};
        for (int bound : {1, 0}) {
          h.opt_active_bound = bound;
          CHECK(c.plan(h, dp) == nullptr && dp.D[0] == D, "D = %d in the bank of three", D);
          check_pack(h, c, dp);
        }
        h.opt_active_bound = 1;
      }
  }

  // randomised calls at the limits: every row lands on a distinct state index of its trajectory
  std::mt19937 rng(7);
  for (int it = 0; it < 2000; ++it) {
    Call c;
    c.count = 1 + (int)(rng() % 3);
    c.b0 = (int)(rng() % (4 - c.count));
    c.stride = 1 + (int)(rng() % EKF_MMAX);
    c.target.assign((size_t)c.count * c.stride, 0);
    c.m.assign(c.count, 0);
    c.z.assign((size_t)c.count * c.stride * 3, 0.25);
    c.R.assign((size_t)c.count * c.stride * 9, 0.0);
    for (size_t f = 0; f < (size_t)c.count * c.stride; ++f) c.R[9 * f] = c.R[9 * f + 4] = c.R[9 * f + 8] = 0.01;
    int d_hi = 0;
    for (int bi = 0; bi < c.count; ++bi) {
      const int nl = (h.n[c.b0 + bi] - 3) / 2;
      c.m[bi] = (int)(rng() % (std::min(c.stride, nl) + 1));
      std::vector<int> pool(nl);
      for (int l = 0; l < nl; ++l) pool[l] = l;
      std::shuffle(pool.begin(), pool.end(), rng);
      int D = 0;
      for (int j = 0; j < c.m[bi]; ++j) {
        int t = pool[j];
        if (j == c.m[bi] / 2 && rng() % 2) t = (rng() % 2) ? EKF_DIRECT_POSE : EKF_DIRECT_POSITION;
        c.target[(size_t)bi * c.stride + j] = t;
        D += t == EKF_DIRECT_POSE ? 3 : 2;
      }
      d_hi = std::max(d_hi, D);
      CHECK(D <= 33, "rows %d", D);
    }
    CHECK(c.plan(h, dp) == nullptr, "random call %d", it);
    CHECK(dp.kpad == ((d_hi + 3) & ~3) && dp.kpad <= DIRECT_ROWS && front_rows_cap(dp.kpad, DIRECT_ROWS) >= dp.kpad, "kpad %d for %d", dp.kpad, d_hi);
    check_pack(h, c, dp);
    for (int bi = 0; bi < c.count; ++bi) {
      std::vector<unsigned char> seen(h.n[c.b0 + bi], 0);
      for (int k = 0; k < DIRECT_ROWS; ++k) {
        const int s = dp.s[(size_t)bi * DIRECT_ROWS + k];
        if (k >= dp.D[bi]) { CHECK(s == -1, "pad"); continue; }
        CHECK(s >= 0 && s < h.n[c.b0 + bi] && !seen[s], "row %d -> %d", k, s);
        seen[s] = 1;
        const int src = dp.src[(size_t)bi * DIRECT_ROWS + k];
        CHECK((src >> 2) < c.m[bi] && (src & 3) < 3, "src %d", src);
      }
    }
  }
  std::printf("%ld checks passed\n", checks);
  return 0;
}
