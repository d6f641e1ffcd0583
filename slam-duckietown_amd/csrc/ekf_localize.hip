// Localisation on a frozen map (ekf_localize_step / ekf_localize_update / ekf_localize_run; gfx950, wave64): the Schmidt-Kalman
// ("consider") form of the range/bearing update.  The landmarks' gain is zero, K = [K_p; 0] with K_p = (P H^T)[0..2] S^-1, while
// the landmarks' uncertainty and their correlations with the pose still enter S = H P H^T + R.  With that gain
//     pose += K_p y,   P(0..2, c) <- P(0..2, c) - K_p (H P)(:, c)  for every column c,   P(a, b) untouched for a, b >= 3
// (the Joseph form (I - K H) P (I - K H)^T + K R K^T restricted to its blocks): rows 0..2 of the stored triangle and the pose
// mean move, nothing else does, no rank is appended and no covariance pass is ever due -- ekf_predict_linear's footprint on the
// measurement side.  Both kernels work on P_base with NOTHING PENDING (the host applies what is pending before the first launch).
//
// A step is linear in a pose column x_c = P(0..2, c), c >= 3, and its coefficients P(t_j.., c) never change, because the
// landmark block does not: prediction x <- G x, observation j (landmark at state indices t_j, t_j + 1)
//     x <- M_j x - K_p,j H_l,j [P(t_j, c); P(t_j + 1, c)],   M_j = I - K_p,j H_p,j
// collapse to   x_new = A x + sum_j B_j [P(t_j, c); P(t_j + 1, c)]   with A <- M_j A, B_i <- M_j B_i (i < j), B_j = -K_p,j H_l,j and
// A = G behind the prediction.  The project's solve + panel split:
//   k_loc_solve  one workgroup of ONE wave per trajectory: gathers the compressed set C = {0, 1, 2, t_j, t_j + 1} (35 positions at
//                most; upper triangle, mirrored, like k_joint), runs the prediction and the sequential chain on X = P(0..2, C)
//                against the constant P(C, C), and leaves the pose mean, the pose block's six stored entries, the record
//                {A, B_j, t_j, m, bound} (ekf_device.h: LocRec) and what the logs read.
//   k_loc_rows   grid (ceil(bound / 256), count), thread = column c >= 3: x_new from the record, no dependency between columns.
// The chain: lane a < c holds column a of X in registers; lanes 0..2 also hold the columns of A and lanes < 2 MMAX the columns of
// the B_i, and every one of these 3-vectors takes the same update  v <- v - K_p (H_p v + H_l w)  with its own "landmark part" w
// (a column of X: P(t_j.., C[a]); a column of A: 0; column k of B_i: e_k for i == j, else 0).  The pose block, the pose mean, H, S
// and K_p are formed by every lane alike (a lone wave: the instruction count is the same).  S^-1 in closed form, fast_recip.
// Sums run in observation order j in both kernels: a trajectory's bits do not depend on its slot or its neighbours.
//
// NIS gate: a rejected observation is skipped -- K_p = 0, M = I, B_j = 0, and k_loc_rows does not read its entries at all (the
// record's mask) --, so the result is BIT-IDENTICAL to the call without it; the gate counter counts it.  q = 0 gives NaN rows as
// on the other paths: the pose comes out NaN and EKF_FLAG_NONFINITE is set.
// `in` is the device copy of the step records, the uploaded stream, or -- on the small-state path, as that path's steps and
// k_predict_pose read theirs -- the pinned ring itself: a record is read once, by lanes.
#include <algorithm>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int LR_THREADS = LOC_THREADS;

// The motion model of src/replay_no_ros.py:368-417 at the pose (x, y, th): the new pose and G[0,2], G[1,2] of its Jacobian
// (a copy of its own: the step kernels keep theirs, whose bits must not move).
struct LocMotion {
  double x, y, th, g0, g1;
};
__device__ __forceinline__ LocMotion loc_motion(double x, double y, double th, double lin, double ang, const DeviceConfig& cfg) {
  LocMotion r{x, y, th, 0.0, 0.0};
  if (cfg.disable_motion_model) return r;
  double s0, c0;
  sincos(th, &s0, &c0);
  if (cfg.enable_circular_interpolation && fabs(ang) > cfg.arc_threshold) {   // :390 arc
    double s1, c1;
    sincos(th + ang, &s1, &c1);
    const double rr = lin / ang;
    r.x += -rr * s0 + rr * s1;
    r.y += rr * c0 - rr * c1;
    r.th = wrap_pi(th + ang);                            // :397
    r.g0 = -rr * c0 + rr * c1;                           // :401
    r.g1 = -rr * s0 + rr * s1;                           // :402
  } else {                                               // :376 straight / :405-417 linear mode
    r.x += lin * c0;
    r.y += lin * s0;
    if (!cfg.enable_circular_interpolation) r.th = th + ang;   // no wrap (:409); :381 keeps theta
    r.g0 = -lin * s0;
    r.g1 = lin * c0;
  }
  return r;
}

// v <- v - K (H_p v + H_l w): one 3-vector of the chain (h: the 2 x 5 Jacobian, k: K_p 3 x 2)
__device__ __forceinline__ void loc_apply(double (&v)[3], double w0, double w1, const double (&h)[2][5], const double (&k)[3][2]) {
  const double u0 = fma(h[0][4], w1, fma(h[0][3], w0, fma(h[0][2], v[2], fma(h[0][1], v[1], h[0][0] * v[0]))));
  const double u1 = fma(h[1][4], w1, fma(h[1][3], w0, fma(h[1][2], v[2], fma(h[1][1], v[1], h[1][0] * v[0]))));
#pragma unroll
  for (int r = 0; r < 3; ++r) v[r] = fma(-k[r][1], u1, fma(-k[r][0], u0, v[r]));
}

__global__ __launch_bounds__(64) void k_loc_solve(double* __restrict__ P, double* __restrict__ mu, const int* __restrict__ nact,
                                                  const StepIn* __restrict__ in, SolveOut* __restrict__ so,
                                                  unsigned* __restrict__ flags, const int* __restrict__ neff_floor,
                                                  LocRec* __restrict__ rec, DeviceConfig cfg, int ld, long pstride) {
  __shared__ double sP[CMAX][CMAX + 1];                  // P(C[r], C[l]) at [r][l]: constant but for its rows / columns 0..2
  __shared__ double sMu[CMAX + 1], sZr[MMAX], sZb[MMAX];
  __shared__ int sC[CMAX + 1], sIdx[MMAX];
  const int b = blockIdx.x, lane = threadIdx.x;
  const StepIn& s = in[b];
  // ---- the record, by lanes (one round trip, also over PCIe) ----
  if (lane < MMAX) {
    sIdx[lane] = s.idx[lane];
    sZr[lane] = s.range[lane];
    sZb[lane] = s.bearing[lane];
  }
  const int sflags = s.flags, n = nact[b];
  const bool do_pred = (sflags & FLAG_PREDICT) != 0;
  int m = ((sflags & FLAG_UPDATE) && cfg.enable_measurement_model) ? s.m : 0;
  m = max(0, min(m, MMAX));
  const double lin = s.lin, ang = s.ang;
  // the active bound: what the host baked into the record, raised to the handle's floor (k_solve's rule)
  const int bound = min(n, max(s.neff, neff_floor[b]));
  const int c = 3 + 2 * m;
  __syncthreads();
  const bool on = lane < c;
  int Cl = lane < 3 ? lane : (on ? 3 + 2 * sIdx[(lane - 3) >> 1] + ((lane - 3) & 1) : 0);
  if (Cl < 0 || Cl >= n) Cl = 0;                         // (a validated record never gets here: no access outside the state)
  if (lane <= CMAX) sC[lane] = Cl;
  double* Pb = P + (long)b * pstride;
  double* mub = mu + (long)b * ld;
  __syncthreads();
  // ---- one round trip: the mean at C, and P(C, C) -- lane l takes column l, the upper triangle is authoritative; every load
  // is issued before the first one is used ----
  const double mu_l = mub[Cl];
  double gv[CMAX];
#pragma unroll
  for (int r = 0; r < CMAX; ++r) {
    gv[r] = 0.0;
    if (r < c && on) {
      const int Cr = sC[r];
      gv[r] = Pb[p_index(ld, min(Cr, Cl), max(Cr, Cl))];
    }
  }
  if (lane <= CMAX) sMu[lane] = mu_l;
  if (on) {
#pragma unroll
    for (int r = 0; r < CMAX; ++r)
      if (r < c) sP[r][lane] = gv[r];
  }
  __syncthreads();
  const int ll = on ? lane : 0;
  double pp[3][3];                                       // the pose block, every lane alike
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) pp[r][q] = sP[min(r, q)][max(r, q)];
  double px = sMu[0], py = sMu[1], pth = sMu[2];
  double xv[3] = {sP[0][ll], sP[1][ll], sP[2][ll]};      // column `lane` of X = P(0..2, C)
  double av[3] = {lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0};   // (lanes 0..2) column `lane` of A
  double bv[3] = {0.0, 0.0, 0.0};                        // (lanes < 2 MMAX) column lane & 1 of B_(lane >> 1)
  const bool nz = cfg.noise != nullptr;
  const NoiseRow nr = nz ? noise_row(cfg, b) : NoiseRow{{cfg.rd[0], cfg.rd[1], cfg.rd[2]}, {cfg.qd[0], cfg.qd[1]}};

  // ---- the prediction: x <- G x, pose block G P_pp G^T + rd (:428-430) ----
  if (do_pred) {
    const LocMotion mo = loc_motion(px, py, pth, lin, ang, cfg);
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
  const bool gate = cfg.gate_rej != nullptr;
  unsigned rmask = 0u;
  for (int j = 0; j < m; ++j) {
    const int a = 3 + 2 * j;
    double h[2][5];
    const LinGeom g = linearize_h(px, py, pth, sMu[a], sMu[a + 1], h);
    double y0, y1;
    innovation(g, sZr[j], sZb[j], y0, y1);
    // the 5 x 5 block on {0, 1, 2, t_j, t_j + 1}: the pose block, X at the landmark's positions, the landmark's own block
    double q5[5][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int q = 0; q < 3; ++q) q5[r][q] = pp[r][q];
      q5[r][3] = q5[3][r] = read_lane(xv[r], a);
      q5[r][4] = q5[4][r] = read_lane(xv[r], a + 1);
    }
    q5[3][3] = sP[a][a];
    q5[3][4] = q5[4][3] = sP[a][a + 1];
    q5[4][4] = sP[a + 1][a + 1];
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
    const double rdet = fast_recip(S00 * S11 - S01 * S10);
    const double i00 = S11 * rdet, i01 = -S01 * rdet, i10 = -S10 * rdet, i11 = S00 * rdet;
    const bool rej = gate && innov_reject(y0, y1, i00, i01, i10, i11, cfg.nis_gate);
    if (lane == 0) {                                     // what the innovation log reads (k_innov_step)
      SolveIter& it = so[b].it[j];
      it.y[0] = y0;
      it.y[1] = y1;
      it.si[0] = i00;
      it.si[1] = i01;
      it.si[2] = i10;
      it.si[3] = i11;
    }
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
    loc_apply(xv, sP[a][ll], sP[a + 1][ll], h, k);
    loc_apply(av, 0.0, 0.0, h, k);
    const bool mine = (lane >> 1) == j;
    loc_apply(bv, mine && !(lane & 1) ? 1.0 : 0.0, mine && (lane & 1) ? 1.0 : 0.0, h, k);
  }

  // ---- what the step leaves ----
  LocRec& o = rec[b];
  if (lane < 3) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o.A[3 * r + lane] = av[r];
  }
  if (lane < 2 * MMAX) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o.B[lane >> 1][2 * r + (lane & 1)] = lane < 2 * m ? bv[r] : 0.0;
  }
  if (lane < MMAX) o.t[lane] = lane < m ? sC[3 + 2 * lane] : 0;
  if (lane == 0) {
    o.m = m;
    o.bound = bound;
    o.rej = rmask;
    o.apply = (do_pred || m > 0) ? 1 : 0;
    so[b].neff = bound;                                  // (the mirror of the host's neff_enq)
    so[b].rej = rmask;
    if (o.apply) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = r; q < 3; ++q) Pb[p_index(ld, r, q)] = pp[r][q];
      mub[0] = px;
      mub[1] = py;
      mub[2] = pth;
      const double big = 1.79769313486231570815e308;
      if (!(fabs(px) <= big && fabs(py) <= big && fabs(pth) <= big)) atomicOr(flags + b, EKF_FLAG_NONFINITE);
    }
    if (gate && rmask) cfg.gate_rej[b] += (unsigned long long)__popc(rmask);
  }
}

// x_new = A x + sum_j B_j [P(t_j, c); P(t_j + 1, c)] for column c of rows 0..2.  The record goes to LDS once per workgroup;
// x (rows 0..2 are contiguous along c: p_col / p_lds, both layouts) and, for c >= t_j, the entries (t_j, c), (t_j + 1, c) are
// coalesced; for c < t_j they are stored mirrored at (c, t_j), (c, t_j + 1): a strided gather of one sector per column.  The
// landmark's own 2 x 2 block comes from its three stored entries.  Four observations' loads are in flight at a time.  Nothing
// outside rows 0..2 is written, and the rows >= 3 it reads are written by nobody.
__global__ __launch_bounds__(LR_THREADS) void k_loc_rows(double* __restrict__ P, const LocRec* __restrict__ rec, int ld,
                                                         long pstride, int b0) {
  __shared__ double sA[9], sB[MMAX][6];
  __shared__ int sT[MMAX];
  const int bi = blockIdx.y, b = b0 + bi, t = threadIdx.x;
  const LocRec& r = rec[b];
  if (!r.apply) return;                                  // (the whole workgroup: the trajectory stays bit for bit)
  const int bound = r.bound, m = min(r.m, MMAX);
  const unsigned rej = r.rej;
  if (blockIdx.x * LR_THREADS >= bound) return;
  if (t < 9) sA[t] = r.A[t];
  if (t < 6 * MMAX) sB[t / 6][t % 6] = r.B[t / 6][t % 6];
  if (t < MMAX) sT[t] = r.t[t];
  __syncthreads();
  const int c = blockIdx.x * LR_THREADS + t;
  if (c < 3 || c >= bound) return;
  double* Pb = P + (long)b * pstride;
  double* pc = Pb + p_col(ld, c);                        // entry (0, c)
  const long lds = p_lds(ld);
  const double x0 = pc[0], x1 = pc[lds], x2 = pc[2 * lds];
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
          p0[u] = Pb[p_index(ld, c, tj)];
          p1[u] = Pb[p_index(ld, c, tj + 1)];
        } else {                                         // the landmark's own block: (t, t), (t, t + 1), (t + 1, t + 1)
          const double d01 = Pb[p_index(ld, tj, tj + 1)];
          p0[u] = c == tj ? Pb[p_index(ld, tj, tj)] : d01;
          p1[u] = c == tj ? d01 : Pb[p_index(ld, tj + 1, tj + 1)];
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
  pc[0] = n0;
  pc[lds] = n1;
  pc[2 * lds] = n2;
}

void launch_loc_solve(hipStream_t st, const BankView& k, double* mu, const StepIn* in, const int* neff_floor, LocRec* rec,
                      const DeviceConfig& cfg) {
  hipLaunchKernelGGL(k_loc_solve, dim3(k.batch), dim3(64), 0, st, k.P, mu, k.nact, in, k.so, k.flags, neff_floor, rec, cfg, k.ld,
                     k.pstride);
}

void launch_loc_rows(hipStream_t st, const BankView& k, const LocRec* rec, int groups) {
  hipLaunchKernelGGL(k_loc_rows, dim3(groups, k.batch), dim3(LR_THREADS), 0, st, k.P, rec, k.ld, k.pstride, 0);
}

}  // namespace ekf
