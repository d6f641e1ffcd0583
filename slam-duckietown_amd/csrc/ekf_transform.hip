// k_transform: move a running filter into another frame, in place (ekf_transform).  Per trajectory a rigid frame g = (t, phi) --
// the old frame expressed in the new one, ekf_join_maps' explicit-mode convention -- with covariance Sigma (or none: the frame
// is known exactly) maps every item c of the filter's own state, the pose included; R = rot(phi), J2 = [[0, -1], [1, 0]]:
//   landmark  l' = t + R l,                    A_c = [I2 | J2 R l],                  B_c = R
//   pose      p' = (t + R p_xy, phi + theta),  A_p = [[I2, J2 R p_xy], [0 0 1]],     B_p = diag(R, 1)     (theta is not wrapped)
//   P'[c1, c2] = B_c1 P[c1, c2] B_c2^T + A_c1 Sigma A_c2^T          (the second term only with a covariance)
// -- the formulas of ekf_join.hip applied to the filter's own items.  Every stored block depends only on itself and on the
// means, so P is read and written once, in place, with no snapshot of it.  The frame terms need the OLD means, which the
// launch's extra workgroup overwrites: the host copies them behind the launch's frame heads first (ekf_host_plan.h: per
// trajectory TF_HEAD doubles {t, phi, has-covariance, Sigma}; behind all heads ld means per trajectory), and every workgroup
// reads them there.
//
// A bandwidth kernel in the manner of k_join and k_copy_traj.  blockIdx.x is the trajectory of the call's range, blockIdx.y <
// tiles_hi a tile of JOIN_ITEMS x JOIN_ITEMS items of the stored upper triangle (ekf_host_plan.h: transform_tile -- item 0 the
// pose, item q landmark q - 1; off-diagonal blocks beyond the active bound are exact zeros, stay so and are not visited),
// blockIdx.y == tiles_hi the workgroup that writes the new means and the pose block.  Lane tid & 31 owns one column item, tid >> 5
// (+ 8 q) its row items: whole 2 x 2 blocks (3 x 2 under the pose, 3 x 3 at it), read and stored through p_col / p_lds -- 8-byte
// accesses, 32 lanes along 512 contiguous bytes of a row; a landmark's two columns may lie in different column panels
// (4095 | 4096): each gets its own p_col.  Only entries of the stored upper triangle are written (of a diagonal block: three).
// Every entry is a fixed sequence of at most 13 products whatever else the launch carries: the same trajectory gives the same
// bits alone or in a bank.  A trajectory whose table row says "not applied" (T = 0 without a covariance) is not touched.
// Plain C++, vector stores only; the 2 x 2 blocks are stored nontemporally (NT: nothing reads them again).  Measured against
// plain stores in one process the two do not differ, 1.209 against 1.206 ms for 32 x N = 2000 (tools/transform_time.py,
// profiles/transform.txt).
#include "ekf_device.h"
#include "ekf_host_plan.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int TF_THREADS = 256;
constexpr int TF_Q = JOIN_ITEMS * JOIN_ITEMS / TF_THREADS;   // row items per thread (4)

// the frame of one trajectory, from the head of its record
struct TfFrame {
  double t[2], phi, c, s;
  double S[3][3];
  bool cov;
};
__device__ __forceinline__ TfFrame tf_frame(const double* __restrict__ fp) {
  TfFrame f;
  f.t[0] = fp[0];
  f.t[1] = fp[1];
  f.phi = fp[2];
  f.cov = fp[3] != 0.0;
  sincos(f.phi, &f.s, &f.c);
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) f.S[u][v] = fp[4 + 3 * u + v];
  return f;
}
// A_c for an item at (x, y) of the old frame: [I2 | J2 R (x, y)] (the pose: with the third row [0 0 1]); and B = diag(R, 1)
__device__ __forceinline__ void tf_jac(const TfFrame& f, double x, double y, double (&A)[3][3], double (&B)[3][3]) {
  const double rx = f.c * x - f.s * y, ry = f.s * x + f.c * y;
  A[0][0] = 1.0; A[0][1] = 0.0; A[0][2] = -ry;
  A[1][0] = 0.0; A[1][1] = 1.0; A[1][2] = rx;
  A[2][0] = 0.0; A[2][1] = 0.0; A[2][2] = 1.0;
  B[0][0] = f.c; B[0][1] = -f.s; B[0][2] = 0.0;
  B[1][0] = f.s; B[1][1] = f.c;  B[1][2] = 0.0;
  B[2][0] = 0.0; B[2][1] = 0.0;  B[2][2] = 1.0;
}
// out = BI Pb BJ^T (+ AI Sigma AJ^T where the frame has a covariance) over the leading NI x NJ, in this order of summation
template <int NI, int NJ>
__device__ __forceinline__ void tf_block(const TfFrame& f, const double (&AI)[3][3], const double (&BI)[3][3], const double (&AJ)[3][3],
                                         const double (&BJ)[3][3], const double (&Pb)[3][3], double (&out)[3][3]) {
#pragma unroll
  for (int r = 0; r < NI; ++r)
#pragma unroll
    for (int d = 0; d < NJ; ++d) {
      double bp = 0.0;
#pragma unroll
      for (int e2 = 0; e2 < NJ; ++e2) {
        double tv = 0.0;
#pragma unroll
        for (int e1 = 0; e1 < NI; ++e1) tv += BI[r][e1] * Pb[e1][e2];
        bp += tv * BJ[d][e2];
      }
      if (f.cov) {
        double acc = 0.0;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const double sv = AI[r][0] * f.S[0][v] + AI[r][1] * f.S[1][v] + AI[r][2] * f.S[2][v];
          acc += sv * AJ[d][v];
        }
        bp = acc + bp;
      }
      out[r][d] = bp;
    }
}

template <bool NT> __device__ __forceinline__ void tf_store(double* p, double v) {
  if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

template <bool NT>
__global__ __launch_bounds__(TF_THREADS) void k_transform(double* __restrict__ Pd, double* __restrict__ mud, const int* __restrict__ tab,
                                                          const double* __restrict__ frames, int tiles_hi, int ld, long pstride) {
  const int* w = tab + TF_WORDS * blockIdx.x;
  const int b = w[0], N = w[1], Ma = w[2], M = 1 + N, tid = threadIdx.x;
  if (!w[3]) return;                                   // T = 0 without a covariance: bit for bit
  const double* fp = frames + (long)blockIdx.x * TF_HEAD;
  const double* mo = frames + (long)gridDim.x * TF_HEAD + (long)blockIdx.x * ld;   // the means before the call
  double* P = Pd + (long)b * pstride;
  const long rd = p_lds(ld);
  const TfFrame f = tf_frame(fp);
  double AP[3][3], BP[3][3];                           // the pose as an item
  tf_jac(f, mo[0], mo[1], AP, BP);

  if ((int)blockIdx.y == tiles_hi) {                   // the new means, the pose and its block
    double* md = mud + (long)b * ld;
    for (int l = tid; l < N; l += TF_THREADS) {
      const double x = mo[3 + 2 * l], y = mo[4 + 2 * l];
      md[3 + 2 * l] = f.t[0] + (f.c * x - f.s * y);
      md[4 + 2 * l] = f.t[1] + (f.s * x + f.c * y);
    }
    if (tid < 2) md[tid] = f.t[tid] + (tid == 0 ? f.c * mo[0] - f.s * mo[1] : f.s * mo[0] + f.c * mo[1]);
    if (tid == 2) md[2] = f.phi + mo[2];
    const int r = tid / 3, c = tid - 3 * r;
    const bool mine = tid < 9 && r <= c;
    double o = 0.0;
    if (mine) {
      double Pr[3][3], out[3][3];
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) Pr[u][v] = u <= v ? P[p_index(ld, u, v)] : P[p_index(ld, v, u)];
      tf_block<3, 3>(f, AP, BP, AP, BP, Pr, out);
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) o = (u == r && v == c) ? out[u][v] : o;
    }
    __syncthreads();                                   // (every lane has read the old block before any of it is overwritten)
    if (mine) P[p_index(ld, r, c)] = o;
    return;
  }

  const int t = blockIdx.y;
  if (t >= transform_tiles(M, Ma)) return;             // (the grid is sized by the launch's largest trajectory)
  int ib, jb;
  transform_tile(Ma, t, &ib, &jb);
  const int J = jb * JOIN_ITEMS + (tid & 31);
  if (J >= M || J < 1) return;
  double AJ[3][3], BJ[3][3];
  tf_jac(f, mo[1 + 2 * J], mo[2 + 2 * J], AJ, BJ);
  const int j0 = 1 + 2 * J;                            // the item's two columns: j0 (odd), j0 + 1
  const long cj[2] = {p_col(ld, j0), p_col(ld, j0 + 1)};

  for (int q = 0; q < TF_Q; ++q) {
    const int I = ib * JOIN_ITEMS + (tid >> 5) + 8 * q;
    if (I > J || !transform_writes(Ma, I, J)) continue;
    double Pr[3][3], out[3][3];
    if (I == 0) {                                      // the pose's three rows
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        Pr[u][0] = P[cj[0] + (long)u * rd];
        Pr[u][1] = P[cj[1] + (long)u * rd];
        Pr[u][2] = 0.0;
      }
      tf_block<3, 2>(f, AP, BP, AJ, BJ, Pr, out);
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        P[cj[0] + (long)u * rd] = out[u][0];
        P[cj[1] + (long)u * rd] = out[u][1];
      }
      continue;
    }
    const int i0 = 1 + 2 * I;                          // the row item's two rows
    double AI[3][3], BI[3][3];
    tf_jac(f, mo[i0], mo[i0 + 1], AI, BI);
    const long r0 = (long)i0 * rd;
    Pr[0][0] = P[cj[0] + r0];
    Pr[0][1] = P[cj[1] + r0];
    Pr[1][1] = P[cj[1] + r0 + rd];
    Pr[1][0] = I == J ? Pr[0][1] : P[cj[0] + r0 + rd]; // (a diagonal block: its entry below the diagonal is the mirrored one)
    Pr[0][2] = Pr[1][2] = Pr[2][0] = Pr[2][1] = Pr[2][2] = 0.0;
    tf_block<2, 2>(f, AI, BI, AJ, BJ, Pr, out);
    tf_store<NT>(&P[cj[0] + r0], out[0][0]);
    tf_store<NT>(&P[cj[1] + r0], out[0][1]);
    if (I != J) tf_store<NT>(&P[cj[0] + r0 + rd], out[1][0]);
    tf_store<NT>(&P[cj[1] + r0 + rd], out[1][1]);
  }
}

void launch_transform(hipStream_t st, bool nt, const BankView& k, double* mu, const int* tab, const double* frames, int count,
                      int tiles_hi) {
  const dim3 grid(count, tiles_hi + 1);
  if (nt)
    hipLaunchKernelGGL(k_transform<true>, grid, dim3(TF_THREADS), 0, st, k.P, mu, tab, frames, tiles_hi, k.ld, k.pstride);
  else
    hipLaunchKernelGGL(k_transform<false>, grid, dim3(TF_THREADS), 0, st, k.P, mu, tab, frames, tiles_hi, k.ld, k.pstride);
}

}  // namespace ekf
