// The pose log (ekf_log_poses, gfx950): the pose mean [x, y, theta] and the pose block P[0:3, 0:3] as they stand after every
// step, kept in a device ring of the last `cap` logged steps -- the trajectory with its covariance over time, which is what
// ATE and a pose-NEES curve against ground truth need (evaluation.py: trajectory_ate, pose_nees_series).
//
// Who writes a row:
//   . fused cadences: the solve workgroup itself, from the mean chain's registers and the block in LDS, behind every step it
//     finishes (k_solve_cad_plog, ekf_cadence.hip);
//   . the small-state path: the workgroup that holds P and the mean in LDS, behind every step of its launch (k_small_stream*_plog,
//     ekf_small.hip);
//   . the per-step kernels (k_solve + k_panels, k_step_split*, k_predict_rc): k_pose_step below, enqueued on the handle's stream
//     behind the step's last pass.  It forms the row from what is in memory then -- the new mean and
//         P(a, b) = P_base[a][b] + sum_k W[a][k] V[k][b] + [a == b] dacc[a]      (a <= b < 3)
//     over the pending ranks, exactly what k_marginals (ekf_marginals.hip) reads for the pose with the same bounds -- reads the
//     filter's buffers only and waits for nothing.  The step kernels are untouched.
#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

// One wave per trajectory: lane = pending rank (kb <= 80: two rounds), a butterfly per entry of the upper triangle.
// kb: the pending rank count rounded up to a whole k-tile (the pad ranks are zero); kb == 0: P_base alone, bit for bit.
__global__ __launch_bounds__(64) void k_pose_step(const double* __restrict__ P, const double* __restrict__ V,
                                                  const double* __restrict__ W, const double* __restrict__ dacc,
                                                  const double* __restrict__ mu, int ld, long pstride, int kb, int batch,
                                                  PoseLog lg) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* Pb = P + (long)b * pstride;
  const double* Vb = V + (long)b * KTOT * ld;
  const double* Wb = W + (long)b * KTOT * ld;
  const int ld16 = ld >> 4;
  double s[6];                                         // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
#pragma unroll
  for (int e = 0; e < 6; ++e) s[e] = 0.0;
  for (int k0 = 0; k0 < kb; k0 += 64) {
    const int k = k0 + lane;
    if (k < kb) {
      const double* v = Vb + (long)k * ld;
      const double v0 = v[0], v1 = v[1], v2 = v[2];
      const double w0 = Wb[wm_index(ld16, k, 0)], w1 = Wb[wm_index(ld16, k, 1)], w2 = Wb[wm_index(ld16, k, 2)];
      s[0] = fma(w0, v0, s[0]);
      s[1] = fma(w0, v1, s[1]);
      s[2] = fma(w0, v2, s[2]);
      s[3] = fma(w1, v1, s[3]);
      s[4] = fma(w1, v2, s[4]);
      s[5] = fma(w2, v2, s[5]);
    }
  }
#pragma unroll
  for (int e = 0; e < 6; ++e)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s[e] += __shfl_xor(s[e], off, 64);
  double* dst = lg.row + ((long)(lg.slot0 % lg.cap) * batch + b) * POSE_ROW;
  if (lane < 3) dst[lane] = mu[(long)b * ld + lane];
  if (lane < 9) {                                      // lane = row-major entry of the block, from its upper triangle
    const int r = lane / 3, c = lane - 3 * r;
    const int a = min(r, c), bb = max(r, c);
    double sum = 0.0;
    if (a == 0) sum = bb == 0 ? s[0] : (bb == 1 ? s[1] : s[2]);
    else if (a == 1) sum = bb == 1 ? s[3] : s[4];
    else sum = s[5];
    double v = Pb[p_index(ld, a, bb)];
    if (kb > 0) {
      v += sum;
      if (a == bb) v += dacc[4 * b + a];
    }
    dst[3 + lane] = v;
  }
}

void launch_pose_step(hipStream_t st, const PendingView& f, const PoseLog& lg) {   // (f: the whole bank, b0 = 0)
  hipLaunchKernelGGL(k_pose_step, dim3(f.count), dim3(64), 0, st, f.P, f.V, f.W, f.dacc, f.mu, f.ld, f.pstride, f.kb, f.count, lg);
}

}  // namespace ekf
