// The likelihood association's arithmetic, stated ONCE for the two kernels that score landmarks against unlabelled range/bearing
// observations: k_assoc_query (ekf_associate.hip: a slot of a filter, pending ranks folded in) and k_hyp_score (ekf_hyp_assoc.hip:
// a hypothesis of a bank on its shared frozen map).  Each forms the 5 x 5 joint covariance p5 and mean m5 of (pose, landmark) its
// own way and calls assoc_score with them: the same p5, m5, noise pair and observations give the same bits in both, which is what
// lets a bank's query be compared bit for bit with the single filter's on an adopted slot.  Also the running two best of an
// observation (AssocBest) and the NaN-ignoring minimum, with ekf_associate's rule for ties and NaN: a strictly smaller score
// replaces, ties stay with the lower landmark index, a NaN never wins, nothing offered leaves -1 / NaN.  gfx950 only.
#pragma once
#include <cmath>

#include "ekf_device.h"

#include "ekf_devfn.h"

namespace ekf {

constexpr int AQ_PART = 9;              // doubles of a partial record: (d, landmark, NIS, ln det S) x 2, smallest NIS

// The running two best of one observation: a candidate that is not NaN takes a place it is strictly smaller than.
struct AssocBest {
  double d[2], nis[2], ld[2], lm[2];
  __device__ __forceinline__ void clear() {
    const double nanv = __builtin_nan("");
    d[0] = d[1] = nis[0] = nis[1] = ld[0] = ld[1] = nanv;
    lm[0] = lm[1] = -1.0;
  }
  __device__ __forceinline__ void offer(double dv, double lv, double nv, double ldv) {
    if (!(dv == dv) || lv < 0.0) return;
    if (lm[0] < 0.0 || dv < d[0]) {
      d[1] = d[0]; lm[1] = lm[0]; nis[1] = nis[0]; ld[1] = ld[0];
      d[0] = dv; lm[0] = lv; nis[0] = nv; ld[0] = ldv;
    } else if (lm[1] < 0.0 || dv < d[1]) {
      d[1] = dv; lm[1] = lv; nis[1] = nv; ld[1] = ldv;
    }
  }
};
__device__ __forceinline__ double nan_min(double a, double v) { return (v == v && (!(a == a) || v < a)) ? v : a; }

// One landmark against the mb <= MMAX observations zr[q], zb[q]: from the joint covariance p5 and mean m5 of (pose, landmark) the
// linearisation, S = H5 P5 H5^T + diag(qd), S^-1 and ln det S (once), then per observation the innovation (bearing wrapped) and
// NIS = y^T S^-1 y into nis_q[q], q < mb (the entries beyond are left as they are).  mb is wave-uniform.
__device__ __forceinline__ void assoc_score(const double (&p5)[5][5], const double (&m5)[5], const double* qd,
                                            const double* __restrict__ zr, const double* __restrict__ zb, int mb,
                                            double (&nis_q)[MMAX], double& logdet) {
  // d, q, z^ and H5 (src/replay_no_ros.py:443-469; q == 0 gives NaN like NumPy's 0/0)
  const double dx = m5[3] - m5[0], dy = m5[4] - m5[1];
  const double qq = dx * dx + dy * dy, sq = sqrt(qq);
  const double zhat1 = atan2(dy, dx) - m5[2];
  double h[2][5];
  h[0][0] = (-sq * dx) / qq;
  h[0][1] = (-sq * dy) / qq;
  h[0][2] = 0.0 / qq;
  h[0][3] = (sq * dx) / qq;
  h[0][4] = (sq * dy) / qq;
  h[1][0] = dy / qq;
  h[1][1] = -dx / qq;
  h[1][2] = -qq / qq;
  h[1][3] = -dy / qq;
  h[1][4] = dx / qq;
  double t5[2][5], S[2][2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int a = 0; a < 5; ++a) acc = fma(h[rr][a], p5[a][c], acc);
      t5[rr][c] = acc;
    }
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int a = 0; a < 5; ++a) acc = fma(t5[rr][a], h[c][a], acc);
      S[rr][c] = acc;
    }
  S[0][0] += qd[0];
  S[1][1] += qd[1];
  const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0];
  const double ia = S[1][1] / det, ib = -S[0][1] / det, ic = -S[1][0] / det, id = S[0][0] / det;
  logdet = log(det);
#pragma unroll
  for (int q = 0; q < MMAX; ++q)
    if (q < mb) {                                        // (uniform)
      const double y0 = zr[q] - sq;
      const double y1 = wrap_pi(zb[q] - zhat1);
      nis_q[q] = innov_nis(y0, y1, ia, ib, ic, id);
    }
}

}  // namespace ekf
