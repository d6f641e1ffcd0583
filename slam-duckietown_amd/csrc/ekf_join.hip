// k_join: append one filter's map to another's on the device (ekf_join_maps) -- sequential map joining and the merge of two maps
// related by a rigid transform.  Per pair (destination A = [r_A; L_A], source B = [r_B; L_B]) a base frame g = (t, phi) with
// covariance Sigma and cross terms G (3 x n_A) maps every item c of B into A's frame, R = rot(phi), J2 = [[0, -1], [1, 0]]:
//   landmark  l' = t + R l,                    A_c = [I2 | J2 R l],                  B_c = R
//   pose      p' = (t + R p_xy, phi + theta),  A_p = [[I2, J2 R p_xy], [0 0 1]],     B_p = diag(R, 1)     (sequential mode only)
//   P'[c1, c2] = A_c1 Sigma A_c2^T + B_c1 P_B[c1, c2] B_c2^T        P'[a, c] = G[:, a]^T A_c^T  for a kept index a of A
// Sequential mode: g is the destination's pose (Sigma = P_A[r, r], G = P_A[r, :]) and is REPLACED by r_A (+) r_B; explicit mode:
// g = T with covariance covT, independent of both maps (G = 0: exact zeros), the destination's pose stays.  The old pose rows,
// pose mean and Sigma are read by every workgroup and overwritten by some, so k_join_snap copies them into the handle's snapshot
// buffer first (JOIN_HEAD doubles {g, -, Sigma, -}, then the three rows, ld apart); in explicit mode the host uploads the head.
//
// A bandwidth kernel in the manner of k_copy_traj.  blockIdx.x is the pair, blockIdx.y < tiles_hi a tile of JOIN_ITEMS x
// JOIN_ITEMS ITEMS of the destination (ekf_host_plan.h: join_tile -- item 0 the pose, item q landmark q - 1), blockIdx.y ==
// tiles_hi the workgroup that writes the new means, the size word and (sequential) the pose block.  Lane tid & 31 owns one column
// item, tid >> 5 (+ 8 q) its row items: whole 2 x 2 blocks (3 x 2 under the pose), read through the SOURCE's layout, stored
// through the DESTINATION's -- 8-byte stores, 32 lanes along 512 contiguous bytes of a row; an appended block starts at an odd
// column, and its two columns may lie in different column panels (4095 | 4096): each gets its own p_col.  Only entries of the
// stored upper triangle are written (of a diagonal block: three).  Every entry is a fixed sequence of at most 13 products
// whatever the pair's place in the launch: the same pair gives the same bits alone or among others.
// The source is only read; a trajectory is never both (plan_join).  Plain C++, vector stores only -- and plain ones: nontemporal
// 8-byte stores were measured, 0.56 against 0.37 ms for 32 pairs of 1500 + 500 landmarks (profiles/join.txt).
#include "ekf_device.h"
#include "ekf_host_plan.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int JN_THREADS = 256;
constexpr int JN_Q = JOIN_ITEMS * JOIN_ITEMS / JN_THREADS;   // row items per thread (4)

// the frame of one pair, from its snapshot head
struct JoinFrame {
  double t[2], phi, c, s;
  double S[3][3];
};
__device__ __forceinline__ JoinFrame join_frame(const double* __restrict__ sp) {
  JoinFrame f;
  f.t[0] = sp[0];
  f.t[1] = sp[1];
  f.phi = sp[2];
  sincos(f.phi, &f.s, &f.c);
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) f.S[u][v] = sp[4 + 3 * u + v];
  return f;
}
// rows 0, 1 of A_c for an item at (x, y) of the source's frame: [I2 | J2 R (x, y)]; and B = R
__device__ __forceinline__ void join_jac(const JoinFrame& f, double x, double y, double (&A)[3][3], double (&B)[3][3]) {
  const double rx = f.c * x - f.s * y, ry = f.s * x + f.c * y;
  A[0][0] = 1.0; A[0][1] = 0.0; A[0][2] = -ry;
  A[1][0] = 0.0; A[1][1] = 1.0; A[1][2] = rx;
  A[2][0] = 0.0; A[2][1] = 0.0; A[2][2] = 1.0;          // (the pose's third row; a landmark has none)
  B[0][0] = f.c; B[0][1] = -f.s; B[0][2] = 0.0;
  B[1][0] = f.s; B[1][1] = f.c;  B[1][2] = 0.0;
  B[2][0] = 0.0; B[2][1] = 0.0;  B[2][2] = 1.0;
}
// out = AI Sigma AJ^T + BI Pb BJ^T over the leading NI x NJ (rows / columns of the two items), in this order of summation
template <int NI, int NJ>
__device__ __forceinline__ void join_block(const double (&AI)[3][3], const double (&BI)[3][3], const double (&AJ)[3][3],
                                           const double (&BJ)[3][3], const double (&S)[3][3], const double (&Pb)[3][3],
                                           double (&out)[3][3]) {
#pragma unroll
  for (int r = 0; r < NI; ++r)
#pragma unroll
    for (int d = 0; d < NJ; ++d) {
      double acc = 0.0;
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const double sv = AI[r][0] * S[0][v] + AI[r][1] * S[1][v] + AI[r][2] * S[2][v];
        acc += sv * AJ[d][v];
      }
      double bp = 0.0;
#pragma unroll
      for (int e2 = 0; e2 < NJ; ++e2) {
        double tv = 0.0;
#pragma unroll
        for (int e1 = 0; e1 < NI; ++e1) tv += BI[r][e1] * Pb[e1][e2];
        bp += tv * BJ[d][e2];
      }
      out[r][d] = acc + bp;
    }
}

// (sequential mode) the destination's pose, Sigma and pose rows as they stand before the join
__global__ __launch_bounds__(JN_THREADS) void k_join_snap(const double* __restrict__ Pd, const double* __restrict__ mud,
                                                          const int* __restrict__ tab, double* __restrict__ snap, long ss, int ldd,
                                                          long psd) {
  const int* w = tab + JOIN_PAIR_WORDS * blockIdx.x;
  const int db = w[0], nA = 3 + 2 * w[2];
  const double* P = Pd + (long)db * psd;
  double* sp = snap + (long)blockIdx.x * ss;
  const int tid = threadIdx.x, a = blockIdx.y * JN_THREADS + tid;
  if (a < nA) {
#pragma unroll
    for (int r = 0; r < 3; ++r) sp[JOIN_HEAD + (long)r * ldd + a] = a >= r ? P[p_index(ldd, r, a)] : P[p_index(ldd, a, r)];
  }
  if (blockIdx.y == 0) {
    if (tid < 3) sp[tid] = mud[(long)db * ldd + tid];
    if (tid < 9) {
      const int r = tid / 3, c = tid - 3 * r;
      sp[4 + tid] = r <= c ? P[p_index(ldd, r, c)] : P[p_index(ldd, c, r)];
    }
  }
}

__global__ __launch_bounds__(JN_THREADS) void k_join(const double* __restrict__ Ps, double* __restrict__ Pd,
                                                     const double* __restrict__ mus, double* __restrict__ mud, int* __restrict__ nd,
                                                     const int* __restrict__ tab, const double* __restrict__ snap, long ss, int seq,
                                                     int tiles_hi, int lds, long pss, int ldd, long psd) {
  const int* w = tab + JOIN_PAIR_WORDS * blockIdx.x;
  const int db = w[0], sb = w[1], NA = w[2], NB = w[3];
  const int M = 1 + NA + NB, tid = threadIdx.x;
  const double* sp = snap + (long)blockIdx.x * ss;
  const double* G = sp + JOIN_HEAD;                    // (sequential) G[u][a] = G[u * ldd + a]
  const double* ms = mus + (long)sb * lds;
  const double* Pb = Ps + (long)sb * pss;
  double* Pq = Pd + (long)db * psd;
  const long rs = p_lds(lds), rd = p_lds(ldd);
  const JoinFrame f = join_frame(sp);
  double AP[3][3], BP[3][3];                           // the source's pose as an item (sequential)
  join_jac(f, ms[0], ms[1], AP, BP);

  if ((int)blockIdx.y == tiles_hi) {                   // the new means, the size word, the pose and its block
    double* md = mud + (long)db * ldd;
    for (int lb = tid; lb < NB; lb += JN_THREADS) {
      const double x = ms[3 + 2 * lb], y = ms[4 + 2 * lb];
      md[3 + 2 * (NA + lb)] = f.t[0] + (f.c * x - f.s * y);
      md[4 + 2 * (NA + lb)] = f.t[1] + (f.s * x + f.c * y);
    }
    if (tid == 0) nd[db] = 3 + 2 * (NA + NB);
    if (seq && tid < 9) {
      const int r = tid / 3, c = tid - 3 * r;
      if (tid < 2) md[tid] = f.t[tid] + (tid == 0 ? f.c * ms[0] - f.s * ms[1] : f.s * ms[0] + f.c * ms[1]);
      if (tid == 2) md[2] = f.phi + ms[2];
      if (r <= c) {
        double Pr[3][3], out[3][3];
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int v = 0; v < 3; ++v) Pr[u][v] = u <= v ? Pb[p_index(lds, u, v)] : Pb[p_index(lds, v, u)];
        join_block<3, 3>(AP, BP, AP, BP, f.S, Pr, out);
        double o = 0.0;
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int v = 0; v < 3; ++v) o = (u == r && v == c) ? out[u][v] : o;
        Pq[p_index(ldd, r, c)] = o;
      }
    }
    return;
  }

  const int t = blockIdx.y;
  if (t >= join_tiles(NA, NB, seq != 0)) return;       // (the grid is sized by the launch's largest pair)
  int ib, jb;
  join_tile(NA, NB, t, &ib, &jb);
  const int J = jb * JOIN_ITEMS + (tid & 31);
  if (J >= M || J < 1) return;
  const bool newJ = J > NA;
  const int lbj = J - 1 - NA;                          // the source's landmark behind a new column item
  double AJ[3][3], BJ[3][3];
  if (newJ) join_jac(f, ms[3 + 2 * lbj], ms[4 + 2 * lbj], AJ, BJ);
  const int j0 = 1 + 2 * J;                            // the item's two columns of the destination: j0 (odd), j0 + 1
  const long cj[2] = {p_col(ldd, j0), p_col(ldd, j0 + 1)};
  const long sj[2] = {newJ ? p_col(lds, 3 + 2 * lbj) : 0, newJ ? p_col(lds, 4 + 2 * lbj) : 0};   // ... and of the source

  for (int q = 0; q < JN_Q; ++q) {
    const int I = ib * JOIN_ITEMS + (tid >> 5) + 8 * q;
    if (I > J || !join_writes(NA, I, J, seq != 0)) continue;
    double out[3][3];
    if (I == 0) {                                      // the pose's three rows
      if (newJ && seq) {
        double Pr[3][3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          Pr[u][0] = Pb[sj[0] + (long)u * rs];
          Pr[u][1] = Pb[sj[1] + (long)u * rs];
          Pr[u][2] = 0.0;
        }
        join_block<3, 2>(AP, BP, AJ, BJ, f.S, Pr, out);
      } else if (newJ) {                               // explicit: the frame is independent of the destination
#pragma unroll
        for (int u = 0; u < 3; ++u) out[u][0] = out[u][1] = 0.0;
      } else {                                         // (sequential) the new pose against a kept landmark: A_p G
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int e = 0; e < 2; ++e)
            out[u][e] = AP[u][0] * G[j0 + e] + AP[u][1] * G[(long)ldd + j0 + e] + AP[u][2] * G[2 * (long)ldd + j0 + e];
      }
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        Pq[cj[0] + (long)u * rd] = out[u][0];
        Pq[cj[1] + (long)u * rd] = out[u][1];
      }
      continue;
    }
    const int i0 = 1 + 2 * I;                          // the row item's two rows of the destination
    if (I > NA) {                                      // new against new: A Sigma A^T + R P_B R^T
      const int lbi = I - 1 - NA;
      double AI[3][3], BI[3][3], Pr[3][3];
      join_jac(f, ms[3 + 2 * lbi], ms[4 + 2 * lbi], AI, BI);
      const long r0 = (long)(3 + 2 * lbi) * rs;
      Pr[0][0] = Pb[sj[0] + r0];
      Pr[0][1] = Pb[sj[1] + r0];
      Pr[1][1] = Pb[sj[1] + r0 + rs];
      Pr[1][0] = I == J ? Pr[0][1] : Pb[sj[0] + r0 + rs];      // (a diagonal block: its entry below the diagonal is the mirrored one)
      Pr[0][2] = Pr[1][2] = Pr[2][0] = Pr[2][1] = Pr[2][2] = 0.0;
      join_block<2, 2>(AI, BI, AJ, BJ, f.S, Pr, out);
    } else if (seq) {                                  // kept against new: G[:, a]^T A_c^T
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int d = 0; d < 2; ++d)
          out[e][d] = G[i0 + e] * AJ[d][0] + G[(long)ldd + i0 + e] * AJ[d][1] + G[2 * (long)ldd + i0 + e] * AJ[d][2];
    } else {
      out[0][0] = out[0][1] = out[1][0] = out[1][1] = 0.0;
    }
    Pq[cj[0] + (long)i0 * rd] = out[0][0];
    Pq[cj[1] + (long)i0 * rd] = out[0][1];
    if (I != J) Pq[cj[0] + (long)(i0 + 1) * rd] = out[1][0];
    Pq[cj[1] + (long)(i0 + 1) * rd] = out[1][1];
  }
}

void launch_join(hipStream_t st, const BankView& src, const BankView& dst, const double* mus, double* mud, const int* tab,
                 double* snap, int pairs, int tiles_hi, int na_hi, bool seq) {
  const long ss = join_snap_doubles(dst.ld, seq);
  if (seq)
    hipLaunchKernelGGL(k_join_snap, dim3(pairs, (3 + 2 * na_hi + JN_THREADS - 1) / JN_THREADS), dim3(JN_THREADS), 0, st, dst.P, mud, tab,
                       snap, ss, dst.ld, dst.pstride);
  hipLaunchKernelGGL(k_join, dim3(pairs, tiles_hi + 1), dim3(JN_THREADS), 0, st, src.P, dst.P, mus, mud, dst.nact, tab, snap, ss,
                     seq ? 1 : 0, tiles_hi, src.ld, src.pstride, dst.ld, dst.pstride);
}

}  // namespace ekf
