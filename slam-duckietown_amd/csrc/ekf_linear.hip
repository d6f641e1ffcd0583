// k_linear: the rank front (ekf_rank_front.h: the steps, and what is left for the covariance pass behind) of a LINEAR
// measurement update (ekf_update_linear; gfx950, wave64), O(n D ns).  The measurement is r = H_s x[s] + v, v ~ N(0, R), over a
// sub-state s = the pose and up to LINEAR_LMAX landmarks (ns <= 35 state indices) with a dense D x ns matrix H_s, D <= LINEAR_ROWS:
//     S = H_s P[s, s] H_s^T + R,   y = r - H_s mu[s] (or y = r),   mu += P[:, s] H_s^T S^-1 y,   P -= P[:, s] H_s^T S^-1 H_s P[s, :].
// What is this kernel's own:
//   1. In LDS: the plan, H_s transposed (HT[j][k] = H_s[k][j], zero beyond D and ns), P[s, s] gathered from the stored upper
//      triangle (the smaller index is the row; p_index covers both layouts), A = P[s, s] H_s^T, S = H_s A + R (R's upper
//      triangle), and y -- in z mode r - H_s mu[s].  Every sum runs over the sub-state in the order given.
//   3. The column of state index i: c = H_s P[s, i] accumulated entry by entry of the sub-state (P[s_j, i] is loaded and spent
//      on the D accumulators at once: the thread holds D values, not ns + D).
// The active bound: the host has raised it over the highest landmark of the sub-state before the launch (a general row ties
// its targets together), so every index of s lies below it; P_base holds exact zeros in the cross terms beyond the OLD bound
// (see include/ekfslam_hip.h), which is what this kernel and the pass behind it then read there.  A plan whose sub-state
// reaches the bound nevertheless is taken as D = 0.
#include <cmath>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"
#include "ekf_rank_front.h"

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

  front_prologue<DP>(b, t, bound, so, dacc, queue, s_ok, invd);
  if (t == 0) s_bad = 0;
  __syncthreads();
  if (t <= LINEAR_NS) {
    const int s = t < ns ? pl[4 + t] : 0;
    sidx[t] = s;
    if (s < 0 || s >= bound) s_bad = 1;                // (never from plan_linear and the raised bound)
  }
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

  // ---- 2. the factor, y's substitutions, NIS and the gate ----
  const bool applied = front_factor_gate<DP, LN_THREADS>(b, t, D, L, invd, yv, xv, s_ok, s_applied, Rm + DP * DP, out, flags);

  // ---- 3. a thread per state index: V, the mean and W ----
  double* Vb = V + (long)b * KTOT * ld;
  double* Wb = W + (long)b * KTOT * ld;
  // (H_s^T is re-read from LDS for every state index, as front_columns re-reads the factor)
  front_columns<DP, LN_THREADS>(t, applied, bound, kpad, ld, Vb, Wb, mub, L, invd, xv,
                                [&](int i, bool live, double (&c)[DP]) __attribute__((always_inline)) {
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
  });
}

void launch_linear(hipStream_t st, int rows_cap, const BankView& k, double* dacc, double* mu, const int* plan, const double* meas,
                   double* out, int kpad, int nsl, int innovation) {
  with_rows_cap<LINEAR_ROWS>(rows_cap, [&](auto dp) {
    hipLaunchKernelGGL((k_linear<decltype(dp)::value>), dim3(k.batch), dim3(LN_THREADS), 0, st, k.P, k.V, k.W, dacc, mu, k.nact, k.so,
                       k.flags, k.queue, plan, meas, out, k.ld, k.pstride, kpad, nsl, innovation);
  });
}

}  // namespace ekf
