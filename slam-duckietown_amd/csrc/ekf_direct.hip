// k_direct: the O(n D^2) front of a DIRECT measurement update (ekf_update_direct; gfx950, wave64).  A direct measurement
// observes state entries themselves -- z = x[s] + v, v ~ N(0, R), s the state indices of a pose fix (x, y, theta), a position
// fix (x, y) or surveyed landmarks (lx, ly) --, so H is a row selection and
//     S = P[s, s] + R,   y = z - mu[s] (theta wrapped),   mu += P[:, s] S^-1 y,   P -= P[:, s] S^-1 P[s, :].
// With U = P[s, :] (D x n) the covariance update is P += W V with V = U and W = -(S^-1 U)^T: the form the covariance pass applies
// to P_base (k_flush / k_flush_rs, ekf_kernels.hip).  This kernel leaves V, W and the mean; the O(n^2) part is that pass.
//
// Called where nothing is pending (the API has flushed), so P is P_base.  One workgroup per trajectory of the BANK (the pass
// behind it covers the bank: trajectories outside the call's range, with m = 0 or rejected get zero ranks, W = -0.0 and
// V = +0.0 -- the pass adds -0.0 to them, the one addend that leaves every stored value, a -0.0 included, bit for bit):
//   1. S = P[s, s] + R in LDS from the stored upper triangle (the smaller index is the row; p_index covers both layouts), y.
//   2. Cholesky of S (D <= 33, lower factor in place; a pivot <= 0 or non-finite fails the trajectory), then in the first
//      wave, a row per lane: L a = y, NIS = a^T a, L^T x = a.  Rows D .. DP - 1 of the compile-time size DP are the identity.
//      The gate: applied = factored and NIS <= gate (a NaN NIS is rejected); a failed factor also raises EKF_FLAG_NONFINITE.
//   3. A thread per state index i: u = U[:, i] gathered into registers, mu[i] += u^T x in place, w = S^-1 u by two
//      substitutions against the LDS factor (broadcast reads), V[k][i] = u[k], W[i][k] = -w[k] (wm_index) for the launch's
//      `kpad` ranks, zeros for i at or beyond the active bound and up to the padded size ld (the pass reads whole tiles).
// The active bound: state indices at or beyond it are correlated with nothing, so a target there has a block-diagonal share
// of S and its update touches only its own 2 x 2 block and mean, which the pass (it stops at the bound) never visits: its rows
// of U are taken as zero in step 3 and one thread applies the block in closed form, P_l <- R_l (P_l + R_l)^-1 P_l (the same
// matrix as P_l - P_l S_l^-1 P_l, without the cancellation at P_l = landmark_init_var >> R_l), in place.
// The kernel also leaves what a solve leaves for the pass behind it: so[b].neff = the bound, the pending pose noise at zero
// (the pass adds dacc to the pose diagonal) and the row-slab pass's queue heads at zero.
#include <cmath>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int DR_THREADS = 512;

template <int DP>
__global__ __launch_bounds__(DR_THREADS) void k_direct(double* __restrict__ P, double* __restrict__ V, double* __restrict__ W,
                                                       double* __restrict__ dacc, double* __restrict__ mu,
                                                       const int* __restrict__ nact, SolveOut* __restrict__ so,
                                                       unsigned* __restrict__ flags, unsigned* __restrict__ queue,
                                                       const int* __restrict__ plan, const double* __restrict__ meas,
                                                       double* __restrict__ out, int ld, long pstride, int kpad) {
  __shared__ double L[DP][DP + 1];
  __shared__ double invd[DP], yv[DP], xv[DP];
  __shared__ int sidx[DP], score[DP], ssrc[DP];
  __shared__ int s_ok, s_applied;
  const int b = blockIdx.x, t = threadIdx.x;
  const int* pl = plan + (long)b * DIRECT_INTS;
  const double* zm = meas + (long)b * DIRECT_DBLS;
  const double* Rm = zm + 3 * MMAX;
  const int D = min(pl[0], DP), n = nact[b], bound = min(pl[1], n);
  double* Pb = P + (long)b * pstride;
  double* mub = mu + (long)b * ld;

  if (t == 0) {
    so[b].neff = bound;                                // what the covariance pass reads as this trajectory's bound
    s_ok = 1;
#pragma unroll
    for (int a = 0; a < 4; ++a) dacc[4 * b + a] = 0.0;
  }
  if (b == 0 && t < 8) queue[t * RS_QSTRIDE] = 0u;     // (as k_solve: the heads of the pass's work queues)
  if (t < DP) {
    const int s = t < D ? pl[2 + t] : -1;
    sidx[t] = s;
    score[t] = s < bound ? s : -1;                     // rows whose target lies beyond the bound: zero in step 3
    ssrc[t] = t < D ? pl[2 + DIRECT_ROWS + t] : 0;
    invd[t] = 1.0;
  }
  __syncthreads();

  // the current P at state indices (a, c): beyond the bound only a landmark's own block is not zero
  auto pcur = [&](int a, int c) {
    const int lo = min(a, c), hi = max(a, c);
    if (hi >= bound && !(lo == hi || (lo >= 3 && ((lo - 3) >> 1) == ((hi - 3) >> 1)))) return 0.0;
    return Pb[p_index(ld, lo, hi)];
  };

  // ---- 1. S and y ----
  for (int e = t; e < DP * DP; e += DR_THREADS) {
    const int k = e / DP, q = e - k * DP;
    double v = k == q ? 1.0 : 0.0;
    if (k < D && q < D) {
      const int fk = ssrc[k] >> 2, rk = ssrc[k] & 3, fq = ssrc[q] >> 2, rq = ssrc[q] & 3;
      v = pcur(sidx[k], sidx[q]) + (fk == fq ? Rm[9 * fk + 3 * min(rk, rq) + max(rk, rq)] : 0.0);
    }
    L[k][q] = v;
  }
  if (t < DP) {
    double y = 0.0;
    if (t < D) {
      y = zm[3 * (ssrc[t] >> 2) + (ssrc[t] & 3)] - mub[sidx[t]];
      if (sidx[t] == 2) y = wrap_pi(y);
    }
    yv[t] = y;
  }

  // ---- 2. Cholesky, lower factor in place ----
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
    for (int e = t; e < DP * DP; e += DR_THREADS) {
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
      const bool applied = D > 0 && ok && nis <= zm[DIRECT_DBLS - 2];
      s_applied = applied ? 1 : 0;
      out[2 * b] = (D > 0 && ok) ? nis : __builtin_nan("");
      out[2 * b + 1] = applied ? 1.0 : 0.0;
      if (D > 0 && (!ok || nis != nis)) atomicOr(flags + b, EKF_FLAG_NONFINITE);
    }
  }
  __syncthreads();
  const bool applied = s_applied != 0;

  // ---- 3. a thread per state index: the mean, V and W ----
  double* Vb = V + (long)b * KTOT * ld;
  double* Wb = W + (long)b * KTOT * ld;
  const int ld16 = ld >> 4;
  for (int i = t; i < ld; i += DR_THREADS) {
    // (the factor is re-read from LDS for every state index: hoisted out of this loop its DP^2 / 2 entries would not fit the
    //  register file)
    asm volatile("" ::: "memory");
    const bool live = applied && i < bound;            // (bound <= n <= ld)
    double u[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const int s = score[k];
      u[k] = (live && s >= 0) ? Pb[p_index(ld, min(s, i), max(s, i))] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < kpad) Vb[(long)k * ld + i] = u[k];
    if (live) {
      double dm = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) dm = fma(u[k], xv[k], dm);
      mub[i] += dm;
#pragma unroll
      for (int j = 0; j < DP; ++j) {                   // L a = u
        asm volatile("" ::: "memory");              // (row j's loads stay behind row j - 1's: see above)
        u[j] *= invd[j];
#pragma unroll
        for (int k = j + 1; k < DP; ++k) u[k] = fma(-L[k][j], u[j], u[k]);
      }
#pragma unroll
      for (int j = DP - 1; j >= 0; --j) {              // L^T w = a
        asm volatile("" ::: "memory");              // (row j's loads stay behind row j - 1's: see above)
        u[j] *= invd[j];
#pragma unroll
        for (int k = 0; k < j; ++k) u[k] = fma(-L[j][k], u[j], u[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < kpad) Wb[wm_index(ld16, k, i)] = live ? -u[k] : -0.0;   // (W = -0, V = +0: the pass adds -0.0, which changes no bit, not even of a stored -0.0)
  }

  // ---- targets beyond the bound: their own block and mean, in closed form ----
  if (applied && t < D && sidx[t] >= bound && (ssrc[t] & 3) == 0) {
    const int a = sidx[t];
    const double* rr = Rm + 9 * (ssrc[t] >> 2);
    const double r00 = rr[0], r01 = rr[1], r11 = rr[4];
    const double p00 = Pb[p_index(ld, a, a)], p01 = Pb[p_index(ld, a, a + 1)], p11 = Pb[p_index(ld, a + 1, a + 1)];
    const double s00 = p00 + r00, s01 = p01 + r01, s11 = p11 + r11;
    const double idet = 1.0 / (s00 * s11 - s01 * s01);
    const double i00 = s11 * idet, i01 = -s01 * idet, i11 = s00 * idet;
    const double x0 = i00 * yv[t] + i01 * yv[t + 1], x1 = i01 * yv[t] + i11 * yv[t + 1];
    mub[a] += p00 * x0 + p01 * x1;
    mub[a + 1] += p01 * x0 + p11 * x1;
    const double m00 = i00 * p00 + i01 * p01, m01 = i00 * p01 + i01 * p11;      // S^-1 P
    const double m10 = i01 * p00 + i11 * p01, m11 = i01 * p01 + i11 * p11;
    Pb[p_index(ld, a, a)] = r00 * m00 + r01 * m10;                              // R S^-1 P, the upper triangle
    Pb[p_index(ld, a, a + 1)] = r00 * m01 + r01 * m11;
    Pb[p_index(ld, a + 1, a + 1)] = r01 * m01 + r11 * m11;
  }
}

void launch_direct(hipStream_t st, int rows_cap, const BankView& k, double* dacc, double* mu, const int* plan, const double* meas,
                   double* out, int kpad) {
  auto go = [&](auto dp) {
    hipLaunchKernelGGL((k_direct<decltype(dp)::value>), dim3(k.batch), dim3(DR_THREADS), 0, st, k.P, k.V, k.W, dacc, mu, k.nact, k.so,
                       k.flags, k.queue, plan, meas, out, k.ld, k.pstride, kpad);
  };
  switch (rows_cap) {
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    default: go(std::integral_constant<int, DIRECT_ROWS>{}); break;
  }
}

}  // namespace ekf
