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
//   k_hyp_weigh   ONE workgroup: w_k = exp(loglik_k - top) over the hypotheses that weigh (finite log-likelihood, no sticky
//                 NONFINITE flag), their sums, the effective sample size and the bank's evidence into a header on the device.
//   k_hyp_plan    ONE workgroup: systematic resampling from that header -- four block-wide scans (the weights; the running maximum
//                 of t_k = ceil(K C_k - u), which makes the offspring counts non-negative and their sum K in ANY summation order;
//                 the dead slots' ranks; the survivors' surplus offspring) over chunks each thread walks in order, re-reading its
//                 weights from L2 instead of holding 64 doubles in registers.  Survivors stay in place; dead slot number i takes
//                 the i-th surplus offspring, found by bisection in the surplus scan.
//   k_hyp_copy    grid (K, column groups): a dead slot takes its ancestor's rows, 16 bytes per lane, and its record; a survivor's
//                 workgroups leave at once.  Every source is a survivor and no survivor's rows are written: no hazard, no second
//                 copy of X.  Every hypothesis's loglik becomes the header's logmean.  NT: nontemporal stores (ekf_copy.hip's); they
//                 bought nothing that holds -- 4095 copies of one source at N = 2000, call + sync: 114.0 us against 111.1 with
//                 plain stores, 48.9 against 49.4 for 1023 (profiles/hyp_resample.txt); the kernel writes 403 MB in 66 .. 70 us.
//   k_hyp_split   the same grid, after the copy: every slot whose ancestor has two or more offspring moves its pose by s L z_k
//                 (L: the lower Cholesky factor of its pose block) and keeps (1 - s^2) of its block and rows, in place.
//   k_hyp_mixture ONE workgroup behind k_hyp_weigh: the bank's pose mixture -- mean, covariance, best hypothesis -- with the header's
//                 ess, evidence and live count into one HypMixRow: ekf_hypotheses_mixture's answer and a row of ekf_hypotheses_run's log.
// k_hyp_plan, k_hyp_copy and k_hyp_split take the resampling's decision on the device (hyp_gate_open: something weighs and ess <
// ess_min): ekf_hypotheses_resample passes +inf, ekf_hypotheses_run the host's fraction * K, and a closed gate writes nothing.
// The active bound of a hypothesis lives on the device: the solve raises it over the landmarks of its record exactly as
// fill_step raises a slot's on the host, so the columns the row launch touches are the ones k_loc_rows would touch.
#include <algorithm>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_host_plan.h"
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

// ---- weights, systematic resampling, split --------------------------------------------------------------------------------------
struct HypAdd {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct HypMax {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// Exclusive scan over the workgroup's threads in thread order (blockDim.x: whole waves, at most 16): a wave scans by shuffles, the
// waves' totals go through sh[16] and every thread combines them in wave order.  *total: the combination of all threads.  The
// order is fixed, so the same inputs give the same bits; integer sums and maxima are exact in any order.
template <class T, class Op>
__device__ __forceinline__ T hyp_block_scan(T v, T ident, Op op, T* sh, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  T inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(inc, d, 64);
    if (lane >= d) inc = op(o, inc);
  }
  T exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = ident;
  __syncthreads();                                       // (sh may still be read by the scan before this one)
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  T off = ident, all = ident;
  for (int q = 0; q < nw; ++q) {
    if (q == wave) off = all;
    all = op(all, sh[q]);
  }
  *total = all;
  return op(off, exc);
}

// A hypothesis weighs where its log-likelihood is finite and its sticky NONFINITE flag is clear.
__device__ __forceinline__ bool hyp_weighs(const HypState& s) {
  return fabs(s.loglik) <= 1.79769313486231570815e308 && !(s.flags & EKF_FLAG_NONFINITE);
}

// The resampling's gate, taken on the device: k_hyp_plan, k_hyp_copy and k_hyp_split act where something weighs and the effective
// sample size has fallen below ess_min -- HypothesisBank.resample_if's comparison of the same two doubles.  ess_min = +inf
// (ekf_hypotheses_resample): wherever something weighs; ess is finite there.
__device__ __forceinline__ bool hyp_gate_open(const HypWeighOut* head, double ess_min) {
  return head->live > 0 && head->ess < ess_min;
}

// ONE workgroup; thread t on the records [t * chunk, (t + 1) * chunk) (chunk * HYP_PLAN_THREADS >= K)
__global__ __launch_bounds__(HYP_PLAN_THREADS) void k_hyp_weigh(const HypState* __restrict__ st, double* __restrict__ w,
                                                                HypWeighOut* __restrict__ head, int K, int chunk) {
  __shared__ double shd[16];
  __shared__ int shi[16];
  const int k0 = min(K, (int)threadIdx.x * chunk), k1 = min(K, k0 + chunk);
  const double ninf = -__builtin_huge_val();
  double mine = ninf, top;
  for (int k = k0; k < k1; ++k)
    if (hyp_weighs(st[k])) mine = fmax(mine, st[k].loglik);
  hyp_block_scan(mine, ninf, HypMax(), shd, &top);
  double s = 0.0, s2 = 0.0;
  int live = 0, last = -1;
  for (int k = k0; k < k1; ++k) {
    const double wk = hyp_weighs(st[k]) ? exp(st[k].loglik - top) : 0.0;
    w[k] = wk;
    if (wk > 0.0) {
      s += wk;
      s2 += wk * wk;
      live += 1;
      last = k;
    }
  }
  double sum, sum2;
  int nlive, nlast;
  hyp_block_scan(s, 0.0, HypAdd(), shd, &sum);
  hyp_block_scan(s2, 0.0, HypAdd(), shd, &sum2);
  hyp_block_scan(live, 0, HypAdd(), shi, &nlive);
  hyp_block_scan(last, -1, HypMax(), shi, &nlast);
  if (threadIdx.x == 0) {
    head->top = top;
    head->sum = sum;
    head->sum2 = sum2;
    head->ess = nlive > 0 ? sum * sum / sum2 : 0.0;
    head->logmean = nlive > 0 ? top + log(sum / (double)K) : ninf;   // (uniform weights: sum == K, the evidence is `top` itself)
    head->live = nlive;
    head->last = nlast;
    head->pad = 0.0;
  }
}

// t_k before the running maximum: K at the last hypothesis that weighs (the cumulative sum ends at 1 by definition, not by
// rounding), else ceil(K C_k - u) inside [0, K]
__device__ __forceinline__ int hyp_raw_t(int k, int last, int K, double run, double total, double u) {
  if (k >= last) return K;
  const double x = ceil((double)K * (run / total) - u);
  return (int)fmin(fmax(x, 0.0), (double)K);
}

// ONE workgroup, the chunks of k_hyp_weigh.  anc / off / exc are written and read back by different threads of the workgroup
// (behind a barrier): no __restrict__ on them.
__global__ __launch_bounds__(HYP_PLAN_THREADS) void k_hyp_plan(const HypWeighOut* __restrict__ head, const double* __restrict__ w,
                                                               int* anc, int* off, int* exc, int K, int chunk, double u,
                                                               double ess_min) {
  __shared__ double shd[16];
  __shared__ int shi[16];
  const int k0 = min(K, (int)threadIdx.x * chunk), k1 = min(K, k0 + chunk);
  if (head->live == 0) {                                 // (the whole workgroup) a degenerate bank: the identity
    for (int k = k0; k < k1; ++k) {
      anc[k] = k;
      off[k] = 1;
    }
    return;
  }
  if (!hyp_gate_open(head, ess_min)) return;             // (the whole workgroup) the gate is closed: nothing is written
  const double total = head->sum;
  const int last = head->last;
  // 1: the weights' scan -- this thread's cumulative sums start at `base`
  double part = 0.0, unused;
  for (int k = k0; k < k1; ++k) part += w[k];
  const double base = hyp_block_scan(part, 0.0, HypAdd(), shd, &unused);
  // 2: the running maximum of t over the hypotheses that weigh
  double run = base;
  int hi = 0, ti;
  for (int k = k0; k < k1; ++k)
    if (w[k] > 0.0) {
      run += w[k];
      hi = max(hi, hyp_raw_t(k, last, K, run, total, u));
    }
  int tprev = hyp_block_scan(hi, 0, HypMax(), shi, &ti);
  // offspring: t_k - t_{k-1}; a hypothesis that weighs nothing carries t on and has none
  run = base;
  int ndead = 0, nextra = 0;
  for (int k = k0; k < k1; ++k) {
    int tk = tprev;
    if (w[k] > 0.0) {
      run += w[k];
      tk = max(tprev, hyp_raw_t(k, last, K, run, total, u));
    }
    const int o = tk - tprev;
    off[k] = o;
    ndead += o == 0 ? 1 : 0;
    nextra += o > 1 ? o - 1 : 0;
    tprev = tk;
  }
  // 3, 4: the dead slots' ranks and the survivors' surplus offspring
  int rank = hyp_block_scan(ndead, 0, HypAdd(), shi, &ti);
  int extra = hyp_block_scan(nextra, 0, HypAdd(), shi, &ti);
  for (int k = k0; k < k1; ++k) {
    const int o = off[k];
    exc[k] = extra;
    if (o >= 1) {
      anc[k] = k;                                        // survivors stay in place
      extra += o - 1;
    }
  }
  __syncthreads();
  // dead slot number `rank` takes surplus offspring number `rank`: the last a with exc[a] <= rank (it has exc[a + 1] > rank, so
  // at least one surplus offspring: a survivor)
  for (int k = k0; k < k1; ++k) {
    if (off[k] != 0) continue;
    int lo = 0, up = K - 1;
    while (lo < up) {
      const int mid = (lo + up + 1) >> 1;
      if (exc[mid] <= rank) lo = mid; else up = mid - 1;
    }
    anc[k] = lo;
    rank += 1;
  }
}

typedef double hyp_d2 __attribute__((ext_vector_type(2)));

// grid (K, column groups of HYP_COPY_COLS): hypothesis blockIdx.x.  X is read (the ancestor's rows) and written (the dead slot's)
// through one pointer; the two never coincide: an ancestor is a survivor, and a survivor's workgroups leave before they store.
// The record travels field by field without loglik, which every hypothesis -- survivors too -- gets from the header.
template <bool NT>
__global__ __launch_bounds__(HYP_THREADS) void k_hyp_copy(HypState* st, double* X, const HypWeighOut* __restrict__ head,
                                                          const int* __restrict__ anc, int ldx, double ess_min) {
  if (!hyp_gate_open(head, ess_min)) return;             // (loglik too stays: the weights carry on to the next step)
  const int k = blockIdx.x, a = anc[k];
  const bool rec = blockIdx.y == 0 && threadIdx.x == 0;
  if (a == k) {
    if (rec) st[k].loglik = head->logmean;
    return;
  }
  const int c = 2 * ((int)blockIdx.y * HYP_THREADS + (int)threadIdx.x);
  if (c < ldx) {
    const double* s = X + (long)a * 3 * ldx + c;
    double* d = X + (long)k * 3 * ldx + c;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const hyp_d2 v = *reinterpret_cast<const hyp_d2*>(s + (long)r * ldx);
      hyp_d2* p = reinterpret_cast<hyp_d2*>(d + (long)r * ldx);
      if (NT) __builtin_nontemporal_store(v, p);
      else *p = v;
    }
  }
  if (rec) {
    const HypState& s = st[a];
    HypState& d = st[k];
    for (int i = 0; i < 3; ++i) d.pose[i] = s.pose[i];
    for (int i = 0; i < 6; ++i) d.blk[i] = s.blk[i];
    d.loglik = head->logmean;
    d.n_obs = s.n_obs;
    d.n_rej = s.n_rej;
    d.flags = s.flags;
    d.bound = s.bound;
  }
}

__device__ __forceinline__ bool hyp_pivot(double d) { return d > 0.0 && d <= 1.79769313486231570815e308; }

// The grid of k_hyp_copy, behind it; a slot touches only itself.  z: K x 3 draws; s: the split, keep = 1 - s^2 (the host's).
__global__ __launch_bounds__(HYP_THREADS) void k_hyp_split(HypState* __restrict__ st, double* __restrict__ X,
                                                           const HypWeighOut* __restrict__ head, const int* __restrict__ anc,
                                                           const int* __restrict__ off, const double* __restrict__ z, int ldx,
                                                           double s, double keep, double ess_min) {
  if (!hyp_gate_open(head, ess_min)) return;
  const int k = blockIdx.x;
  if (off[anc[k]] < 2) return;                           // (the whole workgroup: the slot stays bit for bit)
  const int c = 2 * ((int)blockIdx.y * HYP_THREADS + (int)threadIdx.x);
  if (c < ldx) {
    double* x = X + (long)k * 3 * ldx + c;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      hyp_d2* p = reinterpret_cast<hyp_d2*>(x + (long)r * ldx);
      hyp_d2 v = *p;
      v.x *= keep;
      v.y *= keep;
      *p = v;
    }
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    HypState& h = st[k];
    // the lower Cholesky factor of the block before scaling; a pivot <= 0 or not finite zeroes its column
    double l00 = 0.0, l10 = 0.0, l20 = 0.0, l11 = 0.0, l21 = 0.0, l22 = 0.0;
    if (hyp_pivot(h.blk[0])) {
      l00 = sqrt(h.blk[0]);
      l10 = h.blk[1] / l00;
      l20 = h.blk[2] / l00;
    }
    const double d1 = h.blk[3] - l10 * l10;
    if (hyp_pivot(d1)) {
      l11 = sqrt(d1);
      l21 = (h.blk[4] - l20 * l10) / l11;
    }
    const double d2 = h.blk[5] - l20 * l20 - l21 * l21;
    if (hyp_pivot(d2)) l22 = sqrt(d2);
    const double z0 = z[3 * (long)k], z1 = z[3 * (long)k + 1], z2 = z[3 * (long)k + 2];
    h.pose[0] += s * (l00 * z0);
    h.pose[1] += s * (l10 * z0 + l11 * z1);
    h.pose[2] += s * (l20 * z0 + l21 * z1 + l22 * z2);    // (not wrapped: the motion model takes any heading)
    for (int i = 0; i < 6; ++i) h.blk[i] *= keep;
  }
}

struct HypMin {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; }
};

// ONE workgroup behind k_hyp_weigh, on its chunks: the bank's mixture pose into *row (evaluation.mixture_pose's quantities).
// Two sweeps over the hypotheses with w > 0 -- a dead one may hold NaN and is skipped, not multiplied by 0 --: the weighted sums
// of x, y, sin theta, cos theta, then with the mean known the six stored entries of sum w (blk + d d^T), d's heading wrapped.
// Every sum is a thread's chunk in order, then hyp_block_scan's fixed order: the same bank gives the same bits from any caller.
__global__ __launch_bounds__(HYP_PLAN_THREADS) void k_hyp_mixture(const HypState* __restrict__ st, const double* __restrict__ w,
                                                                  const HypWeighOut* __restrict__ head,
                                                                  HypMixRow* __restrict__ row, int K, int chunk, double ess_min) {
  __shared__ double shd[16];
  __shared__ int shi[16];
  const int k0 = min(K, (int)threadIdx.x * chunk), k1 = min(K, k0 + chunk);
  const double top = head->top, total = head->sum;
  double part[4] = {0.0, 0.0, 0.0, 0.0}, sum[4];
  int first = K, best;
  for (int k = k0; k < k1; ++k) {
    const double wk = w[k];
    if (!(wk > 0.0)) continue;
    const HypState& s = st[k];
    part[0] += wk * s.pose[0];
    part[1] += wk * s.pose[1];
    part[2] += wk * sin(s.pose[2]);
    part[3] += wk * cos(s.pose[2]);
    if (first == K && s.loglik == top) first = k;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) hyp_block_scan(part[i], 0.0, HypAdd(), shd, &sum[i]);
  hyp_block_scan(first, K, HypMin(), shi, &best);
  const double mean[3] = {sum[0] / total, sum[1] / total, atan2(sum[2], sum[3])};
  double cp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cov[6];
  for (int k = k0; k < k1; ++k) {
    const double wk = w[k];
    if (!(wk > 0.0)) continue;
    const HypState& s = st[k];
    const double d[3] = {s.pose[0] - mean[0], s.pose[1] - mean[1], wrap_pi(s.pose[2] - mean[2])};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = a; c < 3; ++c) cp[hyp_blk(a, c)] += wk * (s.blk[hyp_blk(a, c)] + d[a] * d[c]);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) hyp_block_scan(cp[i], 0.0, HypAdd(), shd, &cov[i]);
  if (threadIdx.x == 0) {
    const bool any = head->live > 0;
    const double nan = __builtin_nan("");
    for (int i = 0; i < 3; ++i) row->mean[i] = any ? mean[i] : nan;
    for (int i = 0; i < 6; ++i) row->cov[i] = any ? cov[i] / total : nan;
    row->ess = head->ess;
    row->logmean = head->logmean;
    row->live = head->live;
    row->best = any && best < K ? best : -1;
    row->resampled = hyp_gate_open(head, ess_min) ? 1 : 0;
    row->pad0 = 0;
    row->pad = 0.0;
  }
}

void launch_hyp_weigh(hipStream_t st, const HypView& v, const HypResampleView& rs, int chunk) {
  hipLaunchKernelGGL(k_hyp_weigh, dim3(1), dim3(HYP_PLAN_THREADS), 0, st, v.st, rs.w, rs.head, v.count, chunk);
}

void launch_hyp_plan(hipStream_t st, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp) {
  hipLaunchKernelGGL(k_hyp_plan, dim3(1), dim3(HYP_PLAN_THREADS), 0, st, rs.head, rs.w, rs.anc, rs.off, rs.exc, v.count, rp.chunk, rp.u,
                     rp.ess_min);
}

void launch_hyp_copy(hipStream_t st, bool nt, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp) {
  if (nt)
    hipLaunchKernelGGL(k_hyp_copy<true>, dim3(v.count, rp.groups), dim3(HYP_THREADS), 0, st, v.st, v.X, rs.head, rs.anc, v.ldx,
                       rp.ess_min);
  else
    hipLaunchKernelGGL(k_hyp_copy<false>, dim3(v.count, rp.groups), dim3(HYP_THREADS), 0, st, v.st, v.X, rs.head, rs.anc, v.ldx,
                       rp.ess_min);
}

void launch_hyp_split(hipStream_t st, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp, const double* z) {
  hipLaunchKernelGGL(k_hyp_split, dim3(v.count, rp.groups), dim3(HYP_THREADS), 0, st, v.st, v.X, rs.head, rs.anc, rs.off, z, v.ldx,
                     rp.s, rp.keep, rp.ess_min);
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

void launch_hyp_mixture(hipStream_t st, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp, HypMixRow* row) {
  hipLaunchKernelGGL(k_hyp_mixture, dim3(1), dim3(HYP_PLAN_THREADS), 0, st, v.st, rs.w, rs.head, row, v.count, rp.chunk, rp.ess_min);
}

}  // namespace ekf
