// k_linear: the O(n D ns) front of a LINEAR measurement update (ekf_update_linear; gfx950, wave64).  The measurement is
// r = H_s x[s] + v, v ~ N(0, R), over a sub-state s = the pose and up to LINEAR_LMAX landmarks (ns <= 35 state indices) with a
// dense D x ns matrix H_s, D <= LINEAR_ROWS:
//     S = H_s P[s, s] H_s^T + R,   y = r - H_s mu[s] (or y = r),   mu += P[:, s] H_s^T S^-1 y,   P -= P[:, s] H_s^T S^-1 H_s P[s, :].
// With V = H_s P[s, :] (D x n) the covariance update is P += W V, W = -(S^-1 V)^T: the form the covariance pass applies to P_base
// (k_flush / k_flush_rs, ekf_kernels.hip).  This kernel leaves V, W and the mean; the O(n^2) part is that pass.  It is k_direct
// (ekf_direct.hip) with one small dense product in front of S and of every column of V; what is said there holds here.
//
// Called where nothing is pending (the API has flushed), so P is P_base.  One workgroup per trajectory of the BANK (trajectories
// outside the call's range, with D = 0 or rejected get zero ranks, W = -0.0 and V = +0.0: the pass leaves them bit for bit):
//   1. In LDS: the plan, H_s transposed (HT[j][k] = H_s[k][j], zero beyond D and ns), P[s, s] gathered from the stored upper
//      triangle (the smaller index is the row; p_index covers both layouts), A = P[s, s] H_s^T, S = H_s A + R (R's upper
//      triangle), and y -- in z mode r - H_s mu[s].  Every sum runs over the sub-state in the order given.
//   2. Cholesky of S, the two substitutions for y in the first wave, NIS and the gate: k_direct's step 2, copied (a shared
//      device function would have to leave k_direct's machine code, and so its results, as they are; a copy does by itself).
//   3. A thread per state index i: c = H_s P[s, i] accumulated entry by entry of the sub-state (P[s_j, i] is loaded and spent
//      on the D accumulators at once: the thread holds D values, not ns + D), V[k][i] = c[k], mu[i] += c^T x, w = S^-1 c by two
//      substitutions against the LDS factor, W[i][k] = -w[k] (wm_index) for the launch's `kpad` ranks; zeros for i at or
//      beyond the active bound and up to the padded size ld (the pass reads whole tiles).
// The active bound: the host has raised it over the highest landmark of the sub-state before the launch (a general row ties
// its targets together), so every index of s lies below it; P_base holds exact zeros in the cross terms beyond the OLD bound
// (see include/ekfslam_hip.h), which is what this kernel and the pass behind it then read there.  A plan whose sub-state
// reaches the bound nevertheless is taken as D = 0.
// The kernel also leaves what a solve leaves for the pass behind it: so[b].neff = the bound, the pending pose noise at zero
// and the row-slab pass's queue heads at zero.
#include <cmath>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int LN_THREADS = 512;

template <int DP>
__global__ __launch_bounds__(LN_THREADS) void k_linear(double* __restrict__ P, double* __restrict__ V, double* __restrict__ W,
                                                       double* __restrict__ dacc, double* __restrict__ mu,
                                                       const int* __restrict__ nact, SolveOut* __restrict__ so,
                                                       unsigned* __restrict__ flags, unsigned* __restrict__ queue,
                                                       const int* __restrict__ plan, const double* __restrict__ meas,
                                                       double* __restrict__ out, int ld, long pstride, int kpad, int nsl,
                                                       int innovation) {
  __shared__ double L[DP][DP + 1];
  __shared__ double HT[LINEAR_NS][DP];
  __shared__ double A[LINEAR_NS][DP + 1];
  __shared__ double Pss[LINEAR_NS][LINEAR_NS + 1];
  __shared__ double invd[DP], yv[DP], xv[DP];
  __shared__ int sidx[LINEAR_NS + 1];
  __shared__ int s_ok, s_applied, s_bad;
  const int b = blockIdx.x, t = threadIdx.x;
  const int* pl = plan + (long)b * LINEAR_INTS;
  const double* Hm = meas + (long)b * linear_dbls(DP, nsl);
  const double* rm = Hm + DP * nsl;
  const double* Rm = rm + DP;
  const int n = nact[b], bound = min(pl[1], n), ns = max(3, min(min(pl[2], LINEAR_NS), nsl));
  double* Pb = P + (long)b * pstride;
  double* mub = mu + (long)b * ld;

  if (t == 0) {
    so[b].neff = bound;                                // what the covariance pass reads as this trajectory's bound
    s_ok = 1;
    s_bad = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) dacc[4 * b + a] = 0.0;
  }
  if (b == 0 && t < 8) queue[t * RS_QSTRIDE] = 0u;     // (as k_solve: the heads of the pass's work queues)
  __syncthreads();
  if (t <= LINEAR_NS) {
    const int s = t < ns ? pl[4 + t] : 0;
    sidx[t] = s;
    if (s < 0 || s >= bound) s_bad = 1;                // (never from plan_linear and the raised bound)
  }
  if (t < DP) invd[t] = 1.0;
  __syncthreads();
  const int D = s_bad ? 0 : max(0, min(pl[0], DP));

  // ---- 1. H_s^T, P[s, s], A = P[s, s] H_s^T, S = H_s A + R and y ----
  for (int e = t; e < LINEAR_NS * DP; e += LN_THREADS) {
    const int j = e / DP, k = e - j * DP;
    HT[j][k] = (k < D && j < ns) ? Hm[k * nsl + j] : 0.0;
  }
  for (int e = t; e < LINEAR_NS * LINEAR_NS; e += LN_THREADS) {
    const int a = e / LINEAR_NS, c = e - a * LINEAR_NS;
    double v = 0.0;
    if (D > 0 && a < ns && c < ns) v = Pb[p_index(ld, min(sidx[a], sidx[c]), max(sidx[a], sidx[c]))];
    Pss[a][c] = v;
  }
  __syncthreads();
  for (int e = t; e < LINEAR_NS * DP; e += LN_THREADS) {
    const int j = e / DP, k = e - j * DP;
    double acc = 0.0;
    for (int c = 0; c < ns; ++c) acc = fma(Pss[j][c], HT[c][k], acc);
    A[j][k] = acc;
  }
  __syncthreads();
  for (int e = t; e < DP * DP; e += LN_THREADS) {
    const int k = e / DP, q = e - k * DP;
    double v = k == q ? 1.0 : 0.0;
    if (k < D && q < D) {
      double acc = 0.0;
      for (int j = 0; j < ns; ++j) acc = fma(HT[j][k], A[j][q], acc);
      v = acc + Rm[min(k, q) * DP + max(k, q)];
    }
    L[k][q] = v;
  }
  if (t < DP) {
    double y = 0.0;
    if (t < D) {
      y = rm[t];
      if (!innovation) {
        double acc = 0.0;
        for (int j = 0; j < ns; ++j) acc = fma(HT[j][t], mub[sidx[j]], acc);
        y -= acc;
      }
    }
    yv[t] = y;
  }

  // ---- 2. Cholesky, lower factor in place (k_direct's) ----
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
    for (int e = t; e < DP * DP; e += LN_THREADS) {
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
      const bool applied = D > 0 && ok && nis <= Rm[DP * DP];
      s_applied = applied ? 1 : 0;
      out[2 * b] = (D > 0 && ok) ? nis : __builtin_nan("");
      out[2 * b + 1] = applied ? 1.0 : 0.0;
      if (D > 0 && (!ok || nis != nis)) atomicOr(flags + b, EKF_FLAG_NONFINITE);
    }
  }
  __syncthreads();
  const bool applied = s_applied != 0;

  // ---- 3. a thread per state index: V, the mean and W ----
  double* Vb = V + (long)b * KTOT * ld;
  double* Wb = W + (long)b * KTOT * ld;
  const int ld16 = ld >> 4;
  for (int i = t; i < ld; i += LN_THREADS) {
    // (the factor and H_s^T are re-read from LDS for every state index, as k_direct re-reads its factor)
    asm volatile("" ::: "memory");
    const bool live = applied && i < bound;            // (bound <= n <= ld)
    double c[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) c[k] = 0.0;
    if (live) {
#pragma unroll 4
      for (int j = 0; j < ns; ++j) {
        const int s = sidx[j];
        const double p = Pb[p_index(ld, min(s, i), max(s, i))];
#pragma unroll
        for (int k = 0; k < DP; ++k) c[k] = fma(HT[j][k], p, c[k]);
      }
    }
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
        asm volatile("" ::: "memory");              // (row j's loads stay behind row j - 1's)
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
      if (k < kpad) Wb[wm_index(ld16, k, i)] = live ? -c[k] : -0.0;   // (W = -0, V = +0: the pass adds -0.0, which changes no bit)
  }
}

void launch_linear(hipStream_t st, int rows_cap, const BankView& k, double* dacc, double* mu, const int* plan, const double* meas,
                   double* out, int kpad, int nsl, int innovation) {
  auto go = [&](auto dp) {
    hipLaunchKernelGGL((k_linear<decltype(dp)::value>), dim3(k.batch), dim3(LN_THREADS), 0, st, k.P, k.V, k.W, dacc, mu, k.nact, k.so,
                       k.flags, k.queue, plan, meas, out, k.ld, k.pstride, kpad, nsl, innovation);
  };
  switch (rows_cap) {
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    default: go(std::integral_constant<int, LINEAR_ROWS>{}); break;
  }
}

}  // namespace ekf
