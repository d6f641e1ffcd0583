// The arithmetic of a frozen-map (Schmidt-Kalman) step, shared by the kernels that run it: k_loc_solve / k_loc_rows on a slot of a
// handle (ekf_localize.hip) and k_hyp_solve / k_hyp_rows on a hypothesis of a bank (ekf_hypotheses.hip).  The two pairs must give
// the same bits for the same inputs, so there is ONE chain and ONE column update, parameterised on where the pose mean, the pose
// block, the pose rows X = P(0..2, :) and the frozen entries P(a, b), a, b >= 3, come from and on where the results go (`Src`):
//   double mean(int i)                 the mean at state index i
//   double cov(int lo, int hi)         the stored entry P(lo, hi), lo <= hi
//   void obs(lane, j, y0, y1, i00, i01, i10, i11, det, rej)   observation j's innovation, the S^-1 used, det S and the gate's
//                                      decision -- called by every lane alike, whether or not the gate rejects
//   void leave(apply, pp, px, py, pth, rmask, bound, gate)    (lane 0) the pose block, the pose mean and the bookkeeping
// See ekf_localize.hip's head for the algebra and the lane layout.  gfx950, wave64: ONE wave runs loc_solve_body.
#pragma once
#include "ekf_device.h"

#include "ekf_devfn.h"

namespace ekf {

// v <- v - K (H_p v + H_l w): one 3-vector of the chain (h: the 2 x 5 Jacobian, k: K_p 3 x 2)
__device__ __forceinline__ void loc_apply(double (&v)[3], double w0, double w1, const double (&h)[2][5], const double (&k)[3][2]) {
  const double u0 = fma(h[0][4], w1, fma(h[0][3], w0, fma(h[0][2], v[2], fma(h[0][1], v[1], h[0][0] * v[0]))));
  const double u1 = fma(h[1][4], w1, fma(h[1][3], w0, fma(h[1][2], v[2], fma(h[1][1], v[1], h[1][0] * v[0]))));
#pragma unroll
  for (int r = 0; r < 3; ++r) v[r] = fma(-k[r][1], u1, fma(-k[r][0], u0, v[r]));
}

// The staging of one wave's solve: P(C[r], C[l]) at sP[r][l] (constant but for its rows / columns 0..2), the mean at C, the
// record's measurements and indices.
struct LocShared {
  double sP[CMAX][CMAX + 1];
  double sMu[CMAX + 1], sZr[MMAX], sZb[MMAX];
  int sC[CMAX + 1], sIdx[MMAX];
};

// One step (one update pass) of one trajectory: the record `s`, the state's size n and the step's active bound; leaves the
// record `o` for the row kernel and hands everything else to `src`.  Every lane of the wave calls it.
template <class Src>
__device__ __forceinline__ void loc_solve_body(const StepIn& s, int n, int bound, Src& src, LocShared& sh, LocRec& o,
                                               const DeviceConfig& cfg, const NoiseRow& nr, bool gate, int lane) {
  // ---- the record, by lanes (one round trip, also over PCIe) ----
  if (lane < MMAX) {
    sh.sIdx[lane] = s.idx[lane];
    sh.sZr[lane] = s.range[lane];
    sh.sZb[lane] = s.bearing[lane];
  }
  const int sflags = s.flags;
  const bool do_pred = (sflags & FLAG_PREDICT) != 0;
  int m = ((sflags & FLAG_UPDATE) && cfg.enable_measurement_model) ? s.m : 0;
  m = max(0, min(m, MMAX));
  const double lin = s.lin, ang = s.ang;
  const int c = 3 + 2 * m;
  __syncthreads();
  const bool on = lane < c;
  int Cl = lane < 3 ? lane : (on ? 3 + 2 * sh.sIdx[(lane - 3) >> 1] + ((lane - 3) & 1) : 0);
  if (Cl < 0 || Cl >= n) Cl = 0;                         // (a validated record never gets here: no access outside the state)
  if (lane <= CMAX) sh.sC[lane] = Cl;
  __syncthreads();
  // ---- one round trip: the mean at C, and P(C, C) -- lane l takes column l, the upper triangle is authoritative; every load
  // is issued before the first one is used ----
  const double mu_l = src.mean(Cl);
  double gv[CMAX];
#pragma unroll
  for (int r = 0; r < CMAX; ++r) {
    gv[r] = 0.0;
    if (r < c && on) {
      const int Cr = sh.sC[r];
      gv[r] = src.cov(min(Cr, Cl), max(Cr, Cl));
    }
  }
  if (lane <= CMAX) sh.sMu[lane] = mu_l;
  if (on) {
#pragma unroll
    for (int r = 0; r < CMAX; ++r)
      if (r < c) sh.sP[r][lane] = gv[r];
  }
  __syncthreads();
  const int ll = on ? lane : 0;
  double pp[3][3];                                       // the pose block, every lane alike
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) pp[r][q] = sh.sP[min(r, q)][max(r, q)];
  double px = sh.sMu[0], py = sh.sMu[1], pth = sh.sMu[2];
  double xv[3] = {sh.sP[0][ll], sh.sP[1][ll], sh.sP[2][ll]};      // column `lane` of X = P(0..2, C)
  double av[3] = {lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0};   // (lanes 0..2) column `lane` of A
  double bv[3] = {0.0, 0.0, 0.0};                        // (lanes < 2 MMAX) column lane & 1 of B_(lane >> 1)

  // ---- the prediction: x <- G x, pose block G P_pp G^T + rd (:428-430) ----
  if (do_pred) {
    const Motion mo = motion_model(px, py, pth, lin, ang, cfg);
    px = mo.x, py = mo.y, pth = mo.th;
    const double g0 = mo.g0, g1 = mo.g1;
    xv[0] = fma(g0, xv[2], xv[0]);
    xv[1] = fma(g1, xv[2], xv[1]);
    av[0] = fma(g0, av[2], av[0]);
    av[1] = fma(g1, av[2], av[1]);
    double T[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      T[0][q] = fma(g0, pp[2][q], pp[0][q]);
      T[1][q] = fma(g1, pp[2][q], pp[1][q]);
      T[2][q] = pp[2][q];
    }
    pp[0][0] = fma(g0, T[0][2], T[0][0]) + nr.rd[0];
    pp[0][1] = pp[1][0] = fma(g1, T[0][2], T[0][1]);
    pp[0][2] = pp[2][0] = T[0][2];
    pp[1][1] = fma(g1, T[1][2], T[1][1]) + nr.rd[1];
    pp[1][2] = pp[2][1] = T[1][2];
    pp[2][2] = T[2][2] + nr.rd[2];
  }

  // ---- the sequential chain (:436-480 with the landmarks' gain zeroed) ----
  unsigned rmask = 0u;
  for (int j = 0; j < m; ++j) {
    const int a = 3 + 2 * j;
    double h[2][5];
    const LinGeom g = linearize_h(px, py, pth, sh.sMu[a], sh.sMu[a + 1], h);
    double y0, y1;
    innovation(g, sh.sZr[j], sh.sZb[j], y0, y1);
    // the 5 x 5 block on {0, 1, 2, t_j, t_j + 1}: the pose block, X at the landmark's positions, the landmark's own block
    double q5[5][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int q = 0; q < 3; ++q) q5[r][q] = pp[r][q];
      q5[r][3] = q5[3][r] = read_lane(xv[r], a);
      q5[r][4] = q5[4][r] = read_lane(xv[r], a + 1);
    }
    q5[3][3] = sh.sP[a][a];
    q5[3][4] = q5[4][3] = sh.sP[a][a + 1];
    q5[4][4] = sh.sP[a + 1][a + 1];
    double hp[2][5];                                     // H P on the five indices
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double v = h[t][0] * q5[0][q];
#pragma unroll
        for (int i = 1; i < 5; ++i) v = fma(h[t][i], q5[i][q], v);
        hp[t][q] = v;
      }
    double S00 = nr.qd[0], S01 = 0.0, S10 = 0.0, S11 = nr.qd[1];   // S = H P H^T + Q (:473)
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      S00 = fma(hp[0][q], h[0][q], S00);
      S01 = fma(hp[0][q], h[1][q], S01);
      S10 = fma(hp[1][q], h[0][q], S10);
      S11 = fma(hp[1][q], h[1][q], S11);
    }
    const double det = S00 * S11 - S01 * S10;
    const double rdet = fast_recip(det);
    const double i00 = S11 * rdet, i01 = -S01 * rdet, i10 = -S10 * rdet, i11 = S00 * rdet;
    const bool rej = gate && innov_reject(y0, y1, i00, i01, i10, i11, cfg.nis_gate);
    src.obs(lane, j, y0, y1, i00, i01, i10, i11, det, rej);
    if (rej) {
      rmask |= 1u << j;
      continue;
    }
    double k[3][2];                                      // K_p = (P H^T)[0..2] S^-1, (P H^T)[r][t] = (H P)[t][r]
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      k[r][0] = hp[0][r] * i00 + hp[1][r] * i10;
      k[r][1] = hp[0][r] * i01 + hp[1][r] * i11;
    }
    px += k[0][0] * y0 + k[0][1] * y1;                   // :476
    py += k[1][0] * y0 + k[1][1] * y1;
    pth += k[2][0] * y0 + k[2][1] * y1;
#pragma unroll
    for (int r = 0; r < 3; ++r)                          // P_pp - K_p (H P)_p: the upper triangle, mirrored
#pragma unroll
      for (int q = r; q < 3; ++q) pp[r][q] = pp[q][r] = fma(-k[r][1], hp[1][q], fma(-k[r][0], hp[0][q], pp[r][q]));
    loc_apply(xv, sh.sP[a][ll], sh.sP[a + 1][ll], h, k);
    loc_apply(av, 0.0, 0.0, h, k);
    const bool mine = (lane >> 1) == j;
    loc_apply(bv, mine && !(lane & 1) ? 1.0 : 0.0, mine && (lane & 1) ? 1.0 : 0.0, h, k);
  }

  // ---- what the step leaves ----
  if (lane < 3) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o.A[3 * r + lane] = av[r];
  }
  if (lane < 2 * MMAX) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o.B[lane >> 1][2 * r + (lane & 1)] = lane < 2 * m ? bv[r] : 0.0;
  }
  if (lane < MMAX) o.t[lane] = lane < m ? sh.sC[3 + 2 * lane] : 0;
  if (lane == 0) {
    o.m = m;
    o.bound = bound;
    o.rej = rmask;
    o.apply = (do_pred || m > 0) ? 1 : 0;
    src.leave(o.apply != 0, pp, px, py, pth, rmask, bound, gate);
  }
}

// x_new = A x + sum_j B_j [P(t_j, c); P(t_j + 1, c)] for column c of rows 0..2: x is read and written at xp[0], xp[xs], xp[2 xs];
// the frozen entries come from Pm (layout `ld`), whose rows 0..2 are not read.  The record is in LDS (sA, sB, sT); the caller
// has checked 3 <= c < bound.  For c > t_j + 1 the entries (t_j, c), (t_j + 1, c) are coalesced; for c < t_j they are stored
// mirrored at (c, t_j), (c, t_j + 1): a strided gather of one sector per column.  The landmark's own 2 x 2 block comes from its
// three stored entries.  Four observations' loads are in flight at a time.
__device__ __forceinline__ void loc_rows_body(double* xp, long xs, const double* Pm, int ld, int c, int m, unsigned rej,
                                              const double (&sA)[9], const double (&sB)[MMAX][6], const int (&sT)[MMAX]) {
  const double* pc = Pm + p_col(ld, c);                  // entry (0, c) of the frozen matrix
  const long lds = p_lds(ld);
  const double x0 = xp[0], x1 = xp[xs], x2 = xp[2 * xs];
  double n0 = fma(sA[2], x2, fma(sA[1], x1, fma(sA[0], x0, 0.0)));
  double n1 = fma(sA[5], x2, fma(sA[4], x1, fma(sA[3], x0, 0.0)));
  double n2 = fma(sA[8], x2, fma(sA[7], x1, fma(sA[6], x0, 0.0)));
  for (int j0 = 0; j0 < m; j0 += 4) {
    double p0[4], p1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      p0[u] = p1[u] = 0.0;
      if (j < m && !((rej >> j) & 1u)) {                 // (workgroup-uniform)
        const int tj = sT[j];
        if (c > tj + 1) {
          p0[u] = pc[(long)tj * lds];
          p1[u] = pc[(long)(tj + 1) * lds];
        } else if (c < tj) {
          p0[u] = Pm[p_index(ld, c, tj)];
          p1[u] = Pm[p_index(ld, c, tj + 1)];
        } else {                                         // the landmark's own block: (t, t), (t, t + 1), (t + 1, t + 1)
          const double d01 = Pm[p_index(ld, tj, tj + 1)];
          p0[u] = c == tj ? Pm[p_index(ld, tj, tj)] : d01;
          p1[u] = c == tj ? d01 : Pm[p_index(ld, tj + 1, tj + 1)];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j < m && !((rej >> j) & 1u)) {
        n0 = fma(sB[j][1], p1[u], fma(sB[j][0], p0[u], n0));
        n1 = fma(sB[j][3], p1[u], fma(sB[j][2], p0[u], n1));
        n2 = fma(sB[j][5], p1[u], fma(sB[j][4], p0[u], n2));
      }
    }
  }
  xp[0] = n0;
  xp[xs] = n1;
  xp[2 * xs] = n2;
}

}  // namespace ekf
