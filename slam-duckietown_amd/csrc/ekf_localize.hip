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
// The chain and the column update themselves are loc_solve_body / loc_rows_body of ekf_loc_chain.h, which the hypothesis bank's
// kernels (ekf_hypotheses.hip) run too -- one arithmetic, the same bits; the kernels here say where a slot's operands live.
// `in` is the device copy of the step records, the uploaded stream, or -- on the small-state path, as that path's steps and
// k_predict_pose read theirs -- the pinned ring itself: a record is read once, by lanes.
#include <algorithm>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"
#include "ekf_loc_chain.h"

namespace ekf {

constexpr int LR_THREADS = LOC_THREADS;

// A slot of a handle as the chain's source (ekf_loc_chain.h): mean, pose block, pose rows and the frozen entries all live in the
// slot's own P_base and mean; what the logs read goes to the slot's SolveOut.
struct LocSlot {
  double* Pb;
  double* mub;
  SolveOut* so;
  unsigned* flags;
  unsigned long long* gate_rej;
  int ld;
  __device__ __forceinline__ double mean(int i) const { return mub[i]; }
  __device__ __forceinline__ double cov(int lo, int hi) const { return Pb[p_index(ld, lo, hi)]; }
  __device__ __forceinline__ void obs(int lane, int j, double y0, double y1, double i00, double i01, double i10, double i11,
                                      double, bool) const {
    if (lane == 0) {                                     // what the innovation log reads (k_innov_step)
      SolveIter& it = so->it[j];
      it.y[0] = y0;
      it.y[1] = y1;
      it.si[0] = i00;
      it.si[1] = i01;
      it.si[2] = i10;
      it.si[3] = i11;
    }
  }
  __device__ __forceinline__ void leave(bool apply, const double (&pp)[3][3], double px, double py, double pth, unsigned rmask,
                                        int bound, bool gate) const {
    so->neff = bound;                                    // (the mirror of the host's neff_enq)
    so->rej = rmask;
    if (apply) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = r; q < 3; ++q) Pb[p_index(ld, r, q)] = pp[r][q];
      mub[0] = px;
      mub[1] = py;
      mub[2] = pth;
      const double big = 1.79769313486231570815e308;
      if (!(fabs(px) <= big && fabs(py) <= big && fabs(pth) <= big)) atomicOr(flags, EKF_FLAG_NONFINITE);
    }
    if (gate && rmask) *gate_rej += (unsigned long long)__popc(rmask);
  }
};

__global__ __launch_bounds__(64) void k_loc_solve(double* __restrict__ P, double* __restrict__ mu, const int* __restrict__ nact,
                                                  const StepIn* __restrict__ in, SolveOut* __restrict__ so,
                                                  unsigned* __restrict__ flags, const int* __restrict__ neff_floor,
                                                  LocRec* __restrict__ rec, DeviceConfig cfg, int ld, long pstride) {
  __shared__ LocShared sh;
  const int b = blockIdx.x, lane = threadIdx.x;
  const StepIn& s = in[b];
  const int n = nact[b];
  // the active bound: what the host baked into the record, raised to the handle's floor (k_solve's rule)
  const int bound = min(n, max(s.neff, neff_floor[b]));
  const bool nz = cfg.noise != nullptr;
  const NoiseRow nr = nz ? noise_row(cfg, b) : NoiseRow{{cfg.rd[0], cfg.rd[1], cfg.rd[2]}, {cfg.qd[0], cfg.qd[1]}};
  const bool gate = cfg.gate_rej != nullptr;
  LocSlot src{P + (long)b * pstride, mu + (long)b * ld, so + b, flags + b, gate ? cfg.gate_rej + b : nullptr, ld};
  loc_solve_body(s, n, bound, src, sh, rec[b], cfg, nr, gate, lane);
}

// x_new = A x + sum_j B_j [P(t_j, c); P(t_j + 1, c)] for column c of rows 0..2 (loc_rows_body).  The record goes to LDS once per
// workgroup; x (rows 0..2 are contiguous along c: p_col / p_lds, both layouts) and the entries (t_j, c), (t_j + 1, c) come from
// the slot's own P_base.  Nothing outside rows 0..2 is written, and the rows >= 3 it reads are written by nobody.
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
  loc_rows_body(Pb + p_col(ld, c), p_lds(ld), Pb, ld, c, m, rej, sA, sB, sT);
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
