// The rank front: what k_direct (ekf_direct.hip) and k_linear (ekf_linear.hip) share.  Both are the O(n D^2) front of a
// measurement update with D stacked rows over a few state indices s,
//     S = C P[s, s] C^T + R,   mu += P[:, s] C^T S^-1 y,   P -= P[:, s] C^T S^-1 C P[s, :]
// (C a row selection for a direct update, a dense D x ns matrix H_s for a linear one).  With V = C P[s, :] (D x n) the
// covariance update is P += W V, W = -(S^-1 V)^T: the form the covariance pass applies to P_base (k_flush / k_flush_rs,
// ekf_kernels.hip).  A front leaves V, W and the mean; the O(n^2) part is that pass.
//
// Called where nothing is pending (the API has flushed), so P is P_base.  One workgroup per trajectory of the BANK (the pass
// behind it covers the bank: trajectories outside the call's range, with D = 0 or rejected get zero ranks, W = -0.0 and
// V = +0.0 -- the pass adds -0.0 to them, the one addend that leaves every stored value, a -0.0 included, bit for bit).  DP is
// the launch's compile-time row cap (with_rows_cap below; ekf_host_plan.h: front_rows_cap), D <= DP the trajectory's own rows:
//   0. front_prologue: what a solve leaves for the pass behind it -- so[b].neff = the active bound, the pending pose noise at
//      zero (the pass adds dacc to the pose diagonal), the row-slab pass's queue heads at zero -- and the start of the factor's
//      state: s_ok = 1, invd = 1 (rows D .. DP - 1 of the factor are the identity).
//   1. The kernel's own: S in LDS (`L`) and y (`yv`).
//   2. front_factor_gate: Cholesky of S (lower factor in place; a pivot <= 0 or non-finite fails the trajectory), then in the
//      first wave, a row per lane: L a = y, NIS = a^T a, L^T x = a (`xv`).  The gate: applied = factored and NIS <= *gate (a NaN
//      NIS is rejected); out[2 b] = NIS (NaN where D = 0 or the factor failed), out[2 b + 1] = applied; a failed factor or a
//      NaN NIS also raises EKF_FLAG_NONFINITE.
//   3. front_columns, a thread per state index i: the kernel's callable forms the column c = V[:, i] in registers (zeros unless
//      `live` = applied and i below the bound); then V[k][i] = c[k], mu[i] += c^T x, w = S^-1 c by two substitutions against the
//      LDS factor (broadcast reads), W[i][k] = -w[k] (wm_index), each for the launch's `kpad` ranks; zeros for i at or beyond
//      the bound and up to the padded size ld (the pass reads whole tiles).
// Every function is forced inline into its kernel: the arithmetic is one sequence of operations whichever kernel runs it, and
// tests/test_gpu_update_rows.py judges every instantiation of both, block by block.
#pragma once
#include <type_traits>

#include "ekf_device.h"

#include "ekf_devfn.h"

namespace ekf {

// (launchers) the run-time row cap as a template argument, as with_mcap: 4, 8, 16 or the kernel's full row count
template <int FULL, typename F>
inline void with_rows_cap(int rows_cap, F&& f) {
  switch (rows_cap) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, FULL>{}); break;
  }
}

// ---- 0. what the pass behind the launch reads, and the factor's initial state (the caller's barrier follows) ----
template <int DP>
__device__ __forceinline__ void front_prologue(int b, int t, int bound, SolveOut* so, double* dacc, unsigned* queue, int& s_ok,
                                               double (&invd)[DP]) {
  if (t == 0) {
    so[b].neff = bound;                                // what the covariance pass reads as this trajectory's bound
    s_ok = 1;
#pragma unroll
    for (int a = 0; a < 4; ++a) dacc[4 * b + a] = 0.0;
  }
  if (b == 0 && t < 8) queue[t * RS_QSTRIDE] = 0u;     // (as k_solve: the heads of the pass's work queues)
  if (t < DP) invd[t] = 1.0;
}

// ---- 2. Cholesky, lower factor in place; y's substitutions, NIS and the gate.  Returns whether the update is applied ----
// (`gate` is read by thread 0 alone.  Called by every thread of the workgroup: it holds barriers.)
template <int DP, int THREADS>
__device__ __forceinline__ bool front_factor_gate(int b, int t, int D, double (&L)[DP][DP + 1], double (&invd)[DP], double (&yv)[DP],
                                                  double (&xv)[DP], int& s_ok, int& s_applied, const double* gate, double* out,
                                                  unsigned* flags) {
  for (int j = 0; j < D; ++j) {
    __syncthreads();
    if (t == 0) {
      const double d = L[j][j];
      if (!(d > 0.0 && d < __builtin_inf())) s_ok = 0;
      const double r = sqrt(d);
      L[j][j] = r;
      invd[j] = 1.0 / r;
    }
    __syncthreads();
    if (t > j && t < D) L[t][j] *= invd[j];
    __syncthreads();
    for (int e = t; e < DP * DP; e += THREADS) {
      const int k = e / DP, q = e - k * DP;
      if (q > j && q <= k && k < D) L[k][q] -= L[k][j] * L[q][j];
    }
  }
  __syncthreads();
  // y's two substitutions in the first wave, row `lane` in a register (the other rows through read_lane)
  if (t < 64) {
    double r = t < DP ? yv[t] : 0.0;
#pragma unroll
    for (int j = 0; j < DP; ++j) {
      const double aj = read_lane(r, j) * invd[j];
      if (t == j) r = aj;
      else if (t > j && t < DP) r -= L[t][j] * aj;
    }
    double nis = 0.0;
#pragma unroll
    for (int j = 0; j < DP; ++j) {
      const double aj = read_lane(r, j);
      nis = fma(aj, aj, nis);
    }
#pragma unroll
    for (int j = DP - 1; j >= 0; --j) {
      const double xj = read_lane(r, j) * invd[j];
      if (t == j) r = xj;
      else if (t < j) r -= L[j][t] * xj;
    }
    if (t < DP) xv[t] = r;
    if (t == 0) {
      const bool ok = s_ok != 0;
      const bool applied = D > 0 && ok && nis <= *gate;
      s_applied = applied ? 1 : 0;
      out[2 * b] = (D > 0 && ok) ? nis : __builtin_nan("");
      out[2 * b + 1] = applied ? 1.0 : 0.0;
      if (D > 0 && (!ok || nis != nis)) atomicOr(flags + b, EKF_FLAG_NONFINITE);
    }
  }
  __syncthreads();
  return s_applied != 0;
}

// ---- 3. a thread per state index i: V, the mean and W from the column `column(i, live, c)` leaves in c (zeros unless live) ----
// The column lives HERE, not in the kernel: as a local array of the function that spends it the compiler keeps it, and the
// substitutions' order of loads and arithmetic, as it did when each kernel held this loop itself -- handed in by reference the
// same arithmetic gave the same bits but, at row cap 16, less than half the registers, fewer factor loads in flight and a
// k_linear 45 % slower (profiles/rank_front.txt).
// (the factor is re-read from LDS for every state index: hoisted out of the loop its DP^2 / 2 entries would not fit the register
//  file, hence the compiler barrier at the head of every iteration and the ones per row)
template <int DP, int THREADS, class Column>
__device__ __forceinline__ void front_columns(int t, bool applied, int bound, int kpad, int ld, double* Vb, double* Wb, double* mub,
                                              double (&L)[DP][DP + 1], double (&invd)[DP], double (&xv)[DP], Column column) {
  const int ld16 = ld >> 4;
  for (int i = t; i < ld; i += THREADS) {
    asm volatile("" ::: "memory");
    const bool live = applied && i < bound;            // (bound <= n <= ld)
    double c[DP];
    column(i, live, c);
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < kpad) Vb[(long)k * ld + i] = c[k];
    if (live) {
      double dm = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) dm = fma(c[k], xv[k], dm);
      mub[i] += dm;
#pragma unroll
      for (int j = 0; j < DP; ++j) {                   // L a = c
        asm volatile("" ::: "memory");                 // (row j's loads stay behind row j - 1's)
        c[j] *= invd[j];
#pragma unroll
        for (int k = j + 1; k < DP; ++k) c[k] = fma(-L[k][j], c[j], c[k]);
      }
#pragma unroll
      for (int j = DP - 1; j >= 0; --j) {              // L^T w = a
        asm volatile("" ::: "memory");
        c[j] *= invd[j];
#pragma unroll
        for (int k = 0; k < j; ++k) c[k] = fma(-L[j][k], c[j], c[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < kpad) Wb[wm_index(ld16, k, i)] = live ? -c[k] : -0.0;   // (W = -0, V = +0: the pass adds -0.0, which changes no bit, not even of a stored -0.0)
  }
}

}  // namespace ekf
