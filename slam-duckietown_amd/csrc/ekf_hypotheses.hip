// A bank of pose hypotheses on one shared frozen map (ekf_hyp_*; gfx950, wave64): ekf_localize_step's algebra with the frozen
// part -- every P(a, b) with a, b >= 3 and the landmark means -- stored ONCE for K hypotheses instead of once per slot.  What
// differs between two hypotheses on the same map is the pose mean, the pose block and the pose rows X = P(0..2, :); a hypothesis
// is a HypState plus X[3][ldx] (ekf_device.h), 24 n bytes where a forked slot costs 8 n^2.
//   k_hyp_solve   one workgroup of ONE wave per hypothesis: loc_solve_body (ekf_loc_chain.h), the chain k_loc_solve runs, gathering
//                 X(:, C) and the pose block from the hypothesis and P(C \ pose, C \ pose) and the landmark means from the map.
//                 A hypothesis's bits depend on its own state, its record and the map, not on K or on its position.  It adds
//                 every observation's log-likelihood term to HypState::loglik, rejected or not, and counts both.
//   k_hyp_rows    grid (column groups, K): loc_rows_body, x read and written in the hypothesis's rows, P(t_j, c) read from the map
//                 -- the same ~m n entries for every hypothesis: they stay in L2.
//   k_hyp_fill    the seed and the reset.  Seed: every hypothesis from rows 0..2, the pose block and the pose mean of the map copy
//                 (the source slot's, as copied at creation); rows 0..2 of the copy are not read again.  Reset: what
//                 ekf_predict_linear with F = 0 does to a slot, for a range of hypotheses: pose and block set, rows zeroed.  Both
//                 clear loglik, the counters and the flags and put the bound back to the map's.
//   k_hyp_compare one thread per stored entry (a, c), 3 <= a <= c < n, of the bank's map and of a slot's P_base, and per landmark
//                 mean: counts the entries whose bits differ (vector atomics on one word).
//   k_hyp_adopt   writes hypothesis k's pose, block and rows into a slot whose frozen part the compare found identical.
// The active bound of a hypothesis lives on the device: the solve raises it over the landmarks of its record exactly as
// fill_step raises a slot's on the host, so the columns the row launch touches are the ones k_loc_rows would touch.
#include <algorithm>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"
#include "ekf_loc_chain.h"

namespace ekf {

// A hypothesis as the chain's source: the pose's mean, block and rows are its own, everything else is the map's.
struct HypSlot {
  HypState* st;
  const double* X;
  const double* Pm;
  const double* mum;
  int ld, ldx;
  double ll;
  int nobs, nrej;
  __device__ __forceinline__ double mean(int i) const { return i < 3 ? st->pose[i] : mum[i]; }
  __device__ __forceinline__ double cov(int lo, int hi) const {
    if (lo >= 3) return Pm[p_index(ld, lo, hi)];
    return hi < 3 ? st->blk[hyp_blk(lo, hi)] : X[(long)lo * ldx + hi];
  }
  __device__ __forceinline__ void obs(int, int, double y0, double y1, double i00, double i01, double i10, double i11, double det,
                                      bool rej) {
    const double term = -0.5 * (innov_nis(y0, y1, i00, i01, i10, i11) + log(det) + 3.67575413281869098616);   // 2 ln 2 pi
    if (fabs(term) <= 1.79769313486231570815e308) ll += term;
    nobs += 1;
    nrej += rej ? 1 : 0;
  }
  __device__ __forceinline__ void leave(bool apply, const double (&pp)[3][3], double px, double py, double pth, unsigned, int bound,
                                        bool) const {
    if (!apply) return;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = r; q < 3; ++q) st->blk[hyp_blk(r, q)] = pp[r][q];
    st->pose[0] = px;
    st->pose[1] = py;
    st->pose[2] = pth;
    const double big = 1.79769313486231570815e308;
    if (!(fabs(px) <= big && fabs(py) <= big && fabs(pth) <= big)) st->flags |= EKF_FLAG_NONFINITE;
    st->bound = bound;
    if (nobs) {
      st->loglik += ll;
      st->n_obs += nobs;
      st->n_rej += nrej;
    }
  }
};

// in: one record for every hypothesis (rec_stride 0) or one each (1); gate: the bank's NIS gate is on (cfg.nis_gate)
__global__ __launch_bounds__(64) void k_hyp_solve(const double* __restrict__ Pm, const double* __restrict__ mum,
                                                  HypState* __restrict__ st, const double* __restrict__ X,
                                                  LocRec* __restrict__ rec, const StepIn* __restrict__ in, int rec_stride,
                                                  DeviceConfig cfg, int gate, int n, int ld, int ldx) {
  __shared__ LocShared sh;
  const int k = blockIdx.x, lane = threadIdx.x;
  const StepIn& s = in[(long)k * rec_stride];
  // the active bound: the hypothesis's, raised over the record's landmarks (fill_step's rule, which the host applies to a slot)
  const int m = ((s.flags & FLAG_UPDATE) && cfg.enable_measurement_model) ? max(0, min(s.m, MMAX)) : 0;
  int bound = st[k].bound;
  for (int j = 0; j < m; ++j) bound = max(bound, 3 + 2 * (s.idx[j] + 1));
  bound = min(bound, n);
  const NoiseRow nr{{cfg.rd[0], cfg.rd[1], cfg.rd[2]}, {cfg.qd[0], cfg.qd[1]}};
  HypSlot src{st + k, X + (long)k * 3 * ldx, Pm, mum, ld, ldx, 0.0, 0, 0};
  loc_solve_body(s, n, bound, src, sh, rec[k], cfg, nr, gate != 0, lane);
}

__global__ __launch_bounds__(HYP_THREADS) void k_hyp_rows(const double* __restrict__ Pm, double* __restrict__ X,
                                                          const LocRec* __restrict__ rec, int ld, int ldx) {
  __shared__ double sA[9], sB[MMAX][6];
  __shared__ int sT[MMAX];
  const int k = blockIdx.y, t = threadIdx.x;
  const LocRec& r = rec[k];
  if (!r.apply) return;                                  // (the whole workgroup: the hypothesis stays bit for bit)
  const int bound = min(r.bound, ldx), m = min(r.m, MMAX);
  const unsigned rej = r.rej;
  if (blockIdx.x * HYP_THREADS >= bound) return;
  if (t < 9) sA[t] = r.A[t];
  if (t < 6 * MMAX) sB[t / 6][t % 6] = r.B[t / 6][t % 6];
  if (t < MMAX) sT[t] = r.t[t];
  __syncthreads();
  const int c = blockIdx.x * HYP_THREADS + t;
  if (c < 3 || c >= bound) return;
  loc_rows_body(X + (long)k * 3 * ldx + c, ldx, Pm, ld, c, m, rej, sA, sB, sT);
}

// grid (ceil(ldx / HYP_THREADS), count): hypothesis k0 + blockIdx.y.  init: count x 12 doubles {pose, cov row-major (its upper
// triangle is read)}, or nullptr: the map copy's own pose, block and rows (the seed).
__global__ __launch_bounds__(HYP_THREADS) void k_hyp_fill(const double* __restrict__ Pm, const double* __restrict__ mum,
                                                          HypState* __restrict__ st, double* __restrict__ X,
                                                          const double* __restrict__ init, int k0, int n, int ld, int ldx,
                                                          int bound0) {
  const int k = k0 + blockIdx.y, c = blockIdx.x * HYP_THREADS + threadIdx.x;
  if (c < ldx) {
    double* x = X + (long)k * 3 * ldx + c;
#pragma unroll
    for (int r = 0; r < 3; ++r) x[(long)r * ldx] = (!init && c >= 3 && c < n) ? Pm[p_index(ld, r, c)] : 0.0;
  }
  if (c == 0) {
    HypState& s = st[k];
    const double* in = init ? init + 12 * (long)blockIdx.y : nullptr;
    for (int r = 0; r < 3; ++r) {
      s.pose[r] = in ? in[r] : mum[r];
      for (int q = r; q < 3; ++q) s.blk[hyp_blk(r, q)] = in ? in[3 + 3 * r + q] : Pm[p_index(ld, r, q)];
    }
    s.loglik = 0.0;
    s.n_obs = s.n_rej = 0;
    s.flags = 0u;
    s.bound = bound0;
    s.pad = 0.0;
  }
}

// grid (ceil(n / HYP_CMP_THREADS), n - 2): row a = 3 + blockIdx.y - 1 of both triangles (blockIdx.y = 0: the landmark means).
__global__ __launch_bounds__(HYP_CMP_THREADS) void k_hyp_compare(const double* __restrict__ Pm, const double* __restrict__ mum,
                                                                 int ldm, const double* __restrict__ Pb,
                                                                 const double* __restrict__ mub, int ldb, int n,
                                                                 unsigned* __restrict__ mismatch) {
  const int c = blockIdx.x * HYP_CMP_THREADS + threadIdx.x;
  if (c < 3 || c >= n) return;
  bool differ;
  if (blockIdx.y == 0) {
    differ = __double_as_longlong(mum[c]) != __double_as_longlong(mub[c]);
  } else {
    const int a = 2 + blockIdx.y;
    if (c < a) return;
    differ = __double_as_longlong(Pm[p_index(ldm, a, c)]) != __double_as_longlong(Pb[p_index(ldb, a, c)]);
  }
  if (differ) atomicAdd(mismatch, 1u);
}

// grid ceil(n / HYP_THREADS): hypothesis k's rows, block and pose into the slot at Pb / mub (layout ldb); so_b.neff: the slot's
// raised bound (the mirror of the host's).  Columns at and beyond the hypothesis's bound hold zeros in X: they are written too.
__global__ __launch_bounds__(HYP_THREADS) void k_hyp_adopt(const HypState* __restrict__ st, const double* __restrict__ X, int ldx,
                                                           double* __restrict__ Pb, double* __restrict__ mub, int ldb, int n,
                                                           SolveOut* __restrict__ so_b, int bound) {
  const int c = blockIdx.x * HYP_THREADS + threadIdx.x;
  if (c >= 3 && c < n) {
    double* pc = Pb + p_col(ldb, c);
    const long lds = p_lds(ldb);
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[(long)r * lds] = X[(long)r * ldx + c];
  }
  if (c == 0) {
    for (int r = 0; r < 3; ++r) {
      mub[r] = st->pose[r];
      for (int q = r; q < 3; ++q) Pb[p_index(ldb, r, q)] = st->blk[hyp_blk(r, q)];
    }
    so_b->neff = bound;
  }
}

void launch_hyp_solve(hipStream_t st, const HypView& v, const StepIn* in, int rec_stride, const DeviceConfig& cfg, bool gate) {
  hipLaunchKernelGGL(k_hyp_solve, dim3(v.count), dim3(64), 0, st, v.map, v.mu, v.st, v.X, v.rec, in, rec_stride, cfg, gate ? 1 : 0,
                     v.n, v.ld, v.ldx);
}

void launch_hyp_rows(hipStream_t st, const HypView& v, int groups) {
  hipLaunchKernelGGL(k_hyp_rows, dim3(groups, v.count), dim3(HYP_THREADS), 0, st, v.map, v.X, v.rec, v.ld, v.ldx);
}

void launch_hyp_fill(hipStream_t st, const HypView& v, const double* init, int k0, int count, int groups, int bound0) {
  hipLaunchKernelGGL(k_hyp_fill, dim3(groups, count), dim3(HYP_THREADS), 0, st, v.map, v.mu, v.st, v.X, init, k0, v.n, v.ld, v.ldx,
                     bound0);
}

void launch_hyp_compare(hipStream_t st, const HypView& v, const double* Pb, const double* mub, int ldb, int groups,
                        unsigned* mismatch) {
  hipLaunchKernelGGL(k_hyp_compare, dim3(groups, v.n - 2), dim3(HYP_CMP_THREADS), 0, st, v.map, v.mu, v.ld, Pb, mub, ldb, v.n,
                     mismatch);
}

void launch_hyp_adopt(hipStream_t st, const HypView& v, int k, double* Pb, double* mub, int ldb, SolveOut* so_b, int bound,
                      int groups) {
  hipLaunchKernelGGL(k_hyp_adopt, dim3(groups), dim3(HYP_THREADS), 0, st, v.st + k, v.X + (long)k * 3 * v.ldx, v.ldx, Pb, mub, ldb,
                     v.n, so_b, bound);
}

}  // namespace ekf
