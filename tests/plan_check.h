// What the stand-alone sanitizer programs (tests/*_check.cpp) share: the CHECK macro with its counter -- a failed check prints
// where and why and ends the run with a non-zero status -- and a HostPlan with the layout ekf_create gives a bank.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ekf_host_plan.h"

static long checks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                              \
      std::fprintf(stderr, "]\n");                                    \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

// A bank of n.size() trajectories of sizes n (active bounds neff, if given: else all active) in a handle of n_max.
inline ekf::HostPlan bank(int n_max, std::vector<int> n, std::vector<int> neff = {}) {
  ekf::HostPlan h;
  h.n_max = n_max;
  h.rows = (n_max + 63) / 64 * 64;
  h.ld = h.rows;
  if (n_max <= 4096) {
    int p2 = 64;
    while (p2 < n_max) p2 *= 2;
    h.ld = p2;
  }
  h.batch = (int)n.size();
  h.pstride = ekf::p_alloc(h.rows, h.ld);
  h.n = n;
  h.neff = neff.empty() ? n : neff;
  h.neff_enq = h.neff;
  return h;
}
