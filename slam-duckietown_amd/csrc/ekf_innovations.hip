// The innovation log (ekf_log_innovations, gfx950): every landmark update's innovation y, its covariance S and the normalised
// innovation squared NIS = y^T S^-1 y, kept in a device ring of the last `cap` logged steps -- the consistency check that needs
// no ground truth (its sum over a run is a log-likelihood).
//
// Every solve already leaves y and the S^-1 it used in global memory: SolveOut::it[j] on the per-step kernels, CadOut::rec at
// cad_rec_off(s) + 14 (y) and + 10 (S^-1) on the fused cadences.  The two kernels here are enqueued on the handle's stream right
// behind a solve launch while the log is on and copy those records out before the next solve reuses them.  They read the
// filter's buffers only and wait for nothing.  (The small-state path keeps no records in memory: k_small_stream's LOG
// instantiations write the log themselves, ekf_small.hip.)
#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

// one entry: S = (S^-1)^-1 and the NIS with the S^-1 the filter actually used
__device__ __forceinline__ void innov_from_si(InnovRec* __restrict__ r, int idx, const double* __restrict__ y,
                                              const double* __restrict__ si, int rejected) {
  const double y0 = y[0], y1 = y[1];
  const double a = si[0], b = si[1], c = si[2], d = si[3];
  const double rdet = 1.0 / (a * d - b * c);
  r->y[0] = y0;
  r->y[1] = y1;
  r->S[0] = d * rdet;
  r->S[1] = -b * rdet;
  r->S[2] = -c * rdet;
  r->S[3] = a * rdet;
  r->nis = innov_nis(y0, y1, a, b, c, d);
  r->idx = idx;
  r->rejected = rejected;
}

// Per-step kernels (k_solve, k_step_split, k_panels_mono's solve workgroup): one update pass of one step per trajectory.  The
// pass's landmarks j < m go to positions jbase + j of the step's row (jbase = 16 p for pass p of a step with more than EKF_MMAX
// landmarks); pass 0 sets the row's count, later passes add to it.  One workgroup of 64 threads per trajectory.  `gate`: the
// NIS gate is on and SolveHead::rej holds the solve's decisions (copied: the log never decides again).
__global__ __launch_bounds__(64) void k_innov_step(const StepIn* __restrict__ in, const SolveOut* __restrict__ so, int meas,
                                                   int gate, int batch, InnovLog lg) {
  const int b = blockIdx.x, j = threadIdx.x;
  const StepIn& s = in[b];
  const int m = ((s.flags & FLAG_UPDATE) && meas) ? min(s.m, MMAX) : 0;
  const long row = lg.slot0 * batch + b;
  if (j == 0) lg.m[row] = lg.jbase == 0 ? m : lg.m[row] + m;
  if (j < m && lg.jbase + j < AMAX)
    innov_from_si(lg.rec + row * AMAX + lg.jbase + j, s.idx[j], so[b].it[j].y, so[b].it[j].si,
                  gate ? (int)((so[b].rej >> j) & 1u) : 0);
}

// A fused cadence (k_solve_cad, any instantiation): trajectory b's slots s0 .. CAD_SLOTS - 1 (right-aligned) belong to the
// touched steps t0 .. t0 + ns - 1 of the uploaded stream -- of the first one the landmarks from j0 on, of the last one those
// below jend -- in order; slot s's record holds S^-1 at cad_rec_off(s) + 10 and y at + 14.  Stream step t is logged in ring
// row (slot0 + t) % cap, landmark j at position j; every touched step's row gets its full count (a step cut by a cadence
// boundary is written by both cadences, its positions from j0 on by the second).  Steps that a later step of the same
// launch overwrites in the ring (cap < ns) are skipped, so no two threads write one place.  One workgroup of 64 threads per
// trajectory; the steps' ranges are cad_step_range's, the prefix sum over them is this kernel's own.
__global__ __launch_bounds__(64) void k_innov_cad(const StepIn* __restrict__ in, const CadPlan* __restrict__ plan,
                                                  const CadOut* __restrict__ co, int meas, int gate, int batch, InnovLog lg) {
  static_assert(CAD_SLOTS <= 64, "one thread per touched step");
  __shared__ int cntS[CAD_SLOTS + 1], loS[CAD_SLOTS + 1], firstS[CAD_SLOTS + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  CadPlan pl = plan[b];
  pl.ns = min(pl.ns, CAD_SLOTS);
  const int ns = pl.ns;
  const int pskip = ns - lg.cap;                             // steps p < pskip are overwritten by step p + cap
  int cnt = 0, lo = 0;
  if (tid < ns) {
    const CadRange r = cad_step_range(pl, in + ((long)(pl.t0 + tid) * batch + b), tid, meas);
    lo = r.lo;
    cnt = r.cnt;
    if (tid >= pskip) lg.m[(long)((lg.slot0 + pl.t0 + tid) % lg.cap) * batch + b] = r.m;
  }
  if (tid <= CAD_SLOTS) {
    cntS[tid] = tid < CAD_SLOTS ? cnt : 0;
    loS[tid] = lo;
  }
  __syncthreads();
  if (tid <= CAD_SLOTS) {
    int f = 0;
    for (int u = 0; u < tid; ++u) f += cntS[u];
    firstS[tid] = f;
  }
  __syncthreads();
  const int nslots = min(firstS[CAD_SLOTS], CAD_SLOTS);
  const int s0 = CAD_SLOTS - nslots;
  const double* rec = co[b].rec;
  const unsigned long long rej = gate ? co[b].rej : 0ull;   // (CadHead::rej: the solve's decisions, by slot)
  for (int e = tid; e < ns * MMAX; e += 64) {
    const int p = e / MMAX, q = e - p * MMAX, j = q - loS[p];
    if (p < pskip || j < 0 || j >= cntS[p]) continue;
    const int sl = s0 + firstS[p] + j;
    if (sl >= CAD_SLOTS) continue;                           // (a plan that disagrees with the records cannot read outside)
    const long t = pl.t0 + p;
    const long row = ((lg.slot0 + t) % lg.cap) * batch + b;
    const double* r = rec + cad_rec_off(sl);
    innov_from_si(lg.rec + row * AMAX + q, in[t * batch + b].idx[q], r + 14, r + 10, (int)((rej >> sl) & 1ull));
  }
}

void launch_innov_step(hipStream_t st, const StepIn* in, const SolveOut* so, int meas, int gate, int batch,
                       const InnovLog& lg) {
  hipLaunchKernelGGL(k_innov_step, dim3(batch), dim3(64), 0, st, in, so, meas, gate, batch, lg);
}

void launch_innov_cad(hipStream_t st, const StepIn* in, const CadPlan* plan, const CadOut* co, int meas, int gate, int batch,
                      const InnovLog& lg) {
  hipLaunchKernelGGL(k_innov_cad, dim3(batch), dim3(64), 0, st, in, plan, co, meas, gate, batch, lg);
}

}  // namespace ekf
