// k_direct: the rank front (ekf_rank_front.h: the steps, and what is left for the covariance pass behind) of a DIRECT
// measurement update (ekf_update_direct; gfx950, wave64).  A direct measurement observes state entries themselves -- z = x[s] + v,
// v ~ N(0, R), s the state indices of a pose fix (x, y, theta), a position fix (x, y) or surveyed landmarks (lx, ly) --, so H is
// a row selection and
//     S = P[s, s] + R,   y = z - mu[s] (theta wrapped),   mu += P[:, s] S^-1 y,   P -= P[:, s] S^-1 P[s, :].
// What is this kernel's own:
//   1. S = P[s, s] + R in LDS from the stored upper triangle (the smaller index is the row; p_index covers both layouts), y.
//   3. The column of state index i: u = P[s, i] gathered into registers.
// The active bound: state indices at or beyond it are correlated with nothing, so a target there has a block-diagonal share
// of S and its update touches only its own 2 x 2 block and mean, which the pass (it stops at the bound) never visits: its rows
// of U are taken as zero in step 3 and one thread applies the block in closed form, P_l <- R_l (P_l + R_l)^-1 P_l (the same
// matrix as P_l - P_l S_l^-1 P_l, without the cancellation at P_l = landmark_init_var >> R_l), in place.
#include <cmath>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"
#include "ekf_rank_front.h"

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

  front_prologue<DP>(b, t, bound, so, dacc, queue, s_ok, invd);
  if (t < DP) {
    const int s = t < D ? pl[2 + t] : -1;
    sidx[t] = s;
    score[t] = s < bound ? s : -1;                     // rows whose target lies beyond the bound: zero in step 3
    ssrc[t] = t < D ? pl[2 + DIRECT_ROWS + t] : 0;
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

  // ---- 2. the factor, y's substitutions, NIS and the gate ----
  const bool applied = front_factor_gate<DP, DR_THREADS>(b, t, D, L, invd, yv, xv, s_ok, s_applied, zm + (DIRECT_DBLS - 2), out, flags);

  // ---- 3. a thread per state index: the mean, V and W ----
  double* Vb = V + (long)b * KTOT * ld;
  double* Wb = W + (long)b * KTOT * ld;
  front_columns<DP, DR_THREADS>(t, applied, bound, kpad, ld, Vb, Wb, mub, L, invd, xv,
                                [&](int i, bool live, double (&u)[DP]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const int s = score[k];
      u[k] = (live && s >= 0) ? Pb[p_index(ld, min(s, i), max(s, i))] : 0.0;
    }
  });

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
  with_rows_cap<DIRECT_ROWS>(rows_cap, [&](auto dp) {
    hipLaunchKernelGGL((k_direct<decltype(dp)::value>), dim3(k.batch), dim3(DR_THREADS), 0, st, k.P, k.V, k.W, dacc, mu, k.nact, k.so,
                       k.flags, k.queue, plan, meas, out, k.ld, k.pstride, kpad);
  });
}

}  // namespace ekf
