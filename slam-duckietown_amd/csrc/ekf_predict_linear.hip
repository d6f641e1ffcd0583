// k_predict_pose: a prediction with the caller's motion model (ekf_predict_linear; gfx950, wave64).  The caller brings the new
// pose mean, F = d(new pose)/d(old pose) (3 x 3) and the process noise Q (3 x 3, positive semi-definite); with G = blockdiag(F, I)
//     mu[0:3] = pose,   P <- G P G^T + Q   i.e.   P[r, r] <- F P[r, r] F^T + Q,   P[r, j] <- F P[r, j]  (j >= 3)
// which touches rows 0..2 of the stored upper triangle and nothing else: O(n) per trajectory with nothing pending, O(n kb) with
// kb ranks pending, and never a covariance pass.  P is the CURRENT covariance (ekf_marginals.hip)
//     P(a, j) = P_base[a][j] + sum_k W[a][k] V[k][j] + [a == j < 3] dacc[a]      (a <= j)
// read with the queries' bounds: kb = the pending ranks as whole k-tiles (the pad ranks are zero), the ranks count for the state
// indices below min(nact[b], so[b].neff), and with kb == 0 nothing is added at all.
//   . Nothing pending (PEND = false): x = P_base(0..2, j) is the current column; F x is written over it.
//   . Ranks pending: the current x is gathered, and (F - I) x is ADDED to P_base(0..2, j): behind it P_base + W V is F x, and W, V
//     and dacc are as they were -- the pass and every step in between apply them as ever.  The pose block gets
//     (F P_rr F^T + Q) - P_rr added to its upper triangle, P_rr the current block, dacc included.
// Products with an entry of F (of F - I) that is zero are skipped -- the entry is the same for the whole workgroup -- and a
// difference that comes out zero is not stored: F = I, Q = 0 leaves every bit of the covariance alone in both forms, signed
// zeros included.
//
// Shape: grid (ceil(n_hi / 256), count), workgroup (x, bi) = 256 state indices of trajectory b0 + bi.  The trajectory's record
// (ekf_device.h: PredictIn) and, with ranks pending, W[0..2][0..kb) go to LDS once per workgroup (wm_index; every later read is a
// broadcast); workgroup x = 0 also stages V[0..kb)[0..2] for the pose block.  Thread j >= 3 loads its three base entries (rows
// 0..2 are contiguous along j: p_col / p_lds, both layouts), adds the ranks -- V[k][j] coalesced along j, four ranks at a time
// with the next four in flight, summed in rank order whatever the slot or the neighbours --, applies F and stores.  Workgroups
// and threads at or beyond the trajectory's bound (the record's: the active bound capped by the size; P_base holds exact zeros
// in rows 0..2 there, and F mixes these rows among themselves only) return before they load.  Thread 0 of workgroup x = 0 alone
// touches the nine entries of the pose block -- it reads the block before it writes it -- and writes the pose mean into the
// mean buffer the next step reads, in place.
// `in` is the device copy of the call's records, or -- on the small-state path, as that path's steps read theirs -- the pinned
// ring itself: a record is read once per workgroup, into LDS.
#include <algorithm>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int PL_THREADS = 256;

// acc + f * x, or acc where f is zero (wave-uniform: f comes from the trajectory's record)
__device__ __forceinline__ double fma_nz(double f, double x, double acc) { return f != 0.0 ? fma(f, x, acc) : acc; }

template <bool PEND>
__global__ __launch_bounds__(PL_THREADS) void k_predict_pose(double* __restrict__ P, const double* __restrict__ V,
                                                             const double* __restrict__ W, const double* __restrict__ dacc,
                                                             double* __restrict__ mu, const int* __restrict__ nact,
                                                             const SolveOut* __restrict__ so, const PredictIn* __restrict__ in,
                                                             int ld, long pstride, int b0, int kb) {
  __shared__ double sF[9], sQ[9], sPose[3];
  __shared__ double sW[PEND ? KTOT : 1][4];            // W[a][k] at [k][a]
  __shared__ double sV[PEND ? KTOT : 1][4];            // (workgroup x = 0) V[k][c] at [k][c], c < 3
  const int bi = blockIdx.y, b = b0 + bi, t = threadIdx.x;
  const PredictIn* rec = in + bi;
  if (!rec->apply) return;                             // (the whole workgroup: the trajectory stays bit for bit)
  const int bound = min(rec->bound, nact[b]);
  const int j = blockIdx.x * PL_THREADS + t;
  if (blockIdx.x > 0 && blockIdx.x * PL_THREADS >= bound) return;
  const int kbound = PEND ? min(bound, so[b].neff) : 0;   // state indices below it take the pending ranks
  double* Pb = P + (long)b * pstride;
  const double* Vb = V + (long)b * KTOT * ld;

  // ---- staging ----
  if (t < 9) {
    sF[t] = rec->F[t];
    sQ[t] = rec->Q[t];
  }
  if (t < 3) sPose[t] = rec->pose[t];
  if (PEND) {
    const double* Wb = W + (long)b * KTOT * ld;
    const int ld16 = ld >> 4;
    for (int e = t; e < 3 * kb; e += PL_THREADS) {
      const int k = e / 3, a = e - 3 * k;
      sW[k][a] = Wb[wm_index(ld16, k, a)];
      if (blockIdx.x == 0) sV[k][a] = Vb[(long)k * ld + a];
    }
  }
  __syncthreads();

  // ---- the pose block and the pose mean ----
  if (blockIdx.x == 0 && t == 0) {
    double B[3][3], X[3][3], T[3][3];                  // the base block, the current block, F X
    for (int a = 0; a < 3; ++a)
      for (int c = a; c < 3; ++c) B[a][c] = B[c][a] = Pb[p_index(ld, a, c)];
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) X[a][c] = B[a][c];
    double F[3][3];
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) F[a][c] = sF[3 * a + c];
    if (PEND) {
      for (int a = 0; a < 3; ++a)
        for (int c = a; c < 3; ++c) {
          double s = 0.0;
          for (int k = 0; k < kb; ++k) s = fma(sW[k][a], sV[k][c], s);
          X[a][c] = B[a][c] + s;
          if (a == c) X[a][c] += dacc[4 * b + a];
          X[c][a] = X[a][c];
        }
    }
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) T[a][c] = fma_nz(F[a][2], X[2][c], fma_nz(F[a][1], X[1][c], fma_nz(F[a][0], X[0][c], -0.0)));
    for (int a = 0; a < 3; ++a)
      for (int c = a; c < 3; ++c) {
        double v = fma_nz(F[c][2], T[a][2], fma_nz(F[c][1], T[a][1], fma_nz(F[c][0], T[a][0], -0.0)));
        const double q = sQ[3 * a + c];
        if (q != 0.0) v += q;
        if (PEND) {
          const double d = v - X[a][c];
          if (d != 0.0) Pb[p_index(ld, a, c)] = B[a][c] + d;
        } else {
          Pb[p_index(ld, a, c)] = v;
        }
      }
    for (int a = 0; a < 3; ++a) mu[(long)b * ld + a] = sPose[a];
  }
  if (j < 3 || j >= bound) return;

  // ---- column j of rows 0..2 ----
  double* pj = Pb + p_col(ld, j);                      // entry (0, j)
  const long lds = p_lds(ld);
  const double x0 = pj[0], x1 = pj[lds], x2 = pj[2 * lds];
  if (PEND) {
    double c0 = x0, c1 = x1, c2 = x2;                  // the current column: the base plus the ranks
    if (j < kbound) {
      const double* vj = Vb + j;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      double va[4], vb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) va[r] = vj[(long)r * ld];
      for (int k0 = 0; k0 < kb; k0 += 8) {             // (kb is a multiple of 4: two groups per round, the second may be absent)
        const bool second = k0 + 4 < kb;
        if (second) {
#pragma unroll
          for (int r = 0; r < 4; ++r) vb[r] = vj[(long)(k0 + 4 + r) * ld];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s0 = fma(sW[k0 + r][0], va[r], s0);
          s1 = fma(sW[k0 + r][1], va[r], s1);
          s2 = fma(sW[k0 + r][2], va[r], s2);
        }
        if (!second) break;
        if (k0 + 8 < kb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) va[r] = vj[(long)(k0 + 8 + r) * ld];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s0 = fma(sW[k0 + 4 + r][0], vb[r], s0);
          s1 = fma(sW[k0 + 4 + r][1], vb[r], s1);
          s2 = fma(sW[k0 + 4 + r][2], vb[r], s2);
        }
      }
      c0 += s0;
      c1 += s1;
      c2 += s2;
    }
    // F - I: what is added to P_base
    const double d0 = fma_nz(sF[2], c2, fma_nz(sF[1], c1, fma_nz(sF[0] - 1.0, c0, -0.0)));
    const double d1 = fma_nz(sF[5], c2, fma_nz(sF[4] - 1.0, c1, fma_nz(sF[3], c0, -0.0)));
    const double d2 = fma_nz(sF[8] - 1.0, c2, fma_nz(sF[7], c1, fma_nz(sF[6], c0, -0.0)));
    if (d0 != 0.0) pj[0] = x0 + d0;
    if (d1 != 0.0) pj[lds] = x1 + d1;
    if (d2 != 0.0) pj[2 * lds] = x2 + d2;
  } else {
    pj[0] = fma_nz(sF[2], x2, fma_nz(sF[1], x1, fma_nz(sF[0], x0, -0.0)));
    pj[lds] = fma_nz(sF[5], x2, fma_nz(sF[4], x1, fma_nz(sF[3], x0, -0.0)));
    pj[2 * lds] = fma_nz(sF[8], x2, fma_nz(sF[7], x1, fma_nz(sF[6], x0, -0.0)));
  }
}

void launch_predict_pose(hipStream_t st, const PendingView& f, double* P, double* mu, const PredictIn* in, int n_hi) {
  const dim3 grid((std::max(n_hi, 3) + PL_THREADS - 1) / PL_THREADS, f.count);
  with_flag(f.kb > 0, [&](auto pend) {
    hipLaunchKernelGGL((k_predict_pose<decltype(pend)::value>), grid, dim3(PL_THREADS), 0, st, P, f.V, f.W, f.dacc, mu, f.nact, f.so, in,
                       f.ld, f.pstride, f.b0, f.kb);
  });
}

}  // namespace ekf
