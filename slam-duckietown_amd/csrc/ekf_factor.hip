// The Cholesky factor of the covariance, P = U^T U with U upper triangular (ekf_factor; gfx950, wave64), and what is done with
// it: U^-T rhs (ekf_factor_solve) and U^T z (ekf_factor_multiply).  Read-only towards the filter: P_base is read once, by
// k_factor_load; everything else works in the handle's factor workspace.
//
// Workspace of a range of trajectories: per trajectory lw x lw doubles, plain row-major with row stride lw = the range's
// largest n rounded up to FB = 64 (trajectory stride lw * lw, a size_t: the workspace is not bound by the 4 GiB of one
// covariance).  A trajectory of size n uses the leading nblk = ceil(n / 64) blocks of rows and columns; its ragged last block
// is padded with an identity diagonal, so every block is full and the padding contributes ln 1 = 0 to the determinant.
// Status words fstat[4 bi] = {info, n, nblk, 0} and the log-determinant flog[bi], written by k_factor_load and k_factor_diag;
// every other launch reads them at its top and leaves a trajectory whose info is set, or whose blocks are used up, alone.
//
// Right-looking blocked Cholesky, block 64.  Per block step k three launches over the whole range (trajectory = a grid
// dimension), ordered by the stream alone -- no wait between workgroups, no counter, no atomic:
//   k_factor_diag   one workgroup per trajectory: the 64 x 64 diagonal block, unblocked in LDS; accumulates the
//                   log-determinant and sets info (LAPACK dpotrf: the 1-based index of the first pivot that is <= 0 or not finite)
//   k_factor_panel  the block's row panel to the right of it, X = U_kk^-T A(k, >k), by substitution: a thread per column, the
//                   column's 64 entries in registers, U_kk^T in LDS (broadcast reads)
//   k_factor_trail  A(i, j) -= U(k, i)^T U(k, j) for the blocks k < i <= j: the rank-64 down-date, the hot kernel.  A
//                   workgroup = 4 waves on a 128 x 128 tile of the trailing triangle, a wave on one 64 x 64 block = 4 x 4
//                   v_mfma_f64_16x16x4_f64 tiles whose accumulators are loaded with A itself.  The panel is staged k-major in
//                   LDS sixteen rows at a time (2 x 18 KB); lane map as in ekf_dense.hip:
//                   A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], C/D col = l & 15, row = (l >> 4) + 4 reg.
// The reduction order of every entry is fixed by its position in the trajectory's own matrix -- never by the range, the bank
// position or the workspace's row stride -- so a trajectory's U is bit-identical across repeats, bank positions and ranges.
//
// ekf_factor_solve (right-looking forward substitution with U^T, the right-hand sides held together: per block step
// k_factor_solve_diag, the block's 64 rows by substitution, and k_factor_solve_update, the row panel's contribution taken off
// every column block to the right) and k_factor_multiply (a workgroup per column block) read U once for all nrhs <= 16
// columns: a block column of U against the vector's rows in chunks of 64 staged in LDS (col_block_dot), in a fixed order.
#include <cmath>

#include "ekf_device.h"
#include "ekf_host_plan.h"
#include "ekf_launch.h"

namespace ekf {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int FT_KH = 16;                // k_factor_trail: panel rows staged at a time
constexpr int FT_LS = 144;               // ... and the row stride of the staged panel (doubles; as k_gemm_f64)
constexpr int FR = FACTOR_RHS;
static_assert(FB == 64 && FR == 16, "thread maps below: 64 columns x 4 row groups, 16 right-hand sides");

// ---- load: the stored upper triangle out of the filter's layout, identity padding, zeros below the diagonal ----
// grid (nblk_hi, nblk_hi, count): workgroup (x, y) = block column x, block row y.
__global__ __launch_bounds__(256) void k_factor_load(const double* __restrict__ P, const int* __restrict__ nact, int ld, long pstride,
                                                     int b0, double* __restrict__ ws, size_t tstride, int lw,
                                                     int* __restrict__ fstat, double* __restrict__ flog) {
  const int bi = blockIdx.z, b = b0 + bi;
  const int n = nact[b], nblk = (n + FB - 1) / FB;
  const int t = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
    fstat[4 * bi + 0] = 0;
    fstat[4 * bi + 1] = n;
    fstat[4 * bi + 2] = nblk;
    fstat[4 * bi + 3] = 0;
    flog[bi] = 0.0;
  }
  if ((int)blockIdx.x >= nblk || (int)blockIdx.y >= nblk) return;
  const double* Pb = P + (long)b * pstride;
  double* A = ws + (size_t)bi * tstride;
  const int j = blockIdx.x * FB + (t & 63);
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int i = blockIdx.y * FB + (t >> 6) + 4 * e;
    double v = 0.0;
    if (i <= j) v = j < n ? Pb[p_index(ld, i, j)] : (i == j ? 1.0 : 0.0);
    A[(size_t)i * lw + j] = v;
  }
}

// ---- the diagonal block of step k ----
__global__ __launch_bounds__(256) void k_factor_diag(double* __restrict__ ws, size_t tstride, int lw, int k, int* __restrict__ fstat,
                                                     double* __restrict__ flog) {
  __shared__ double A[FB][FB + 1];
  const int bi = blockIdx.x;
  int* st = fstat + 4 * bi;
  if (st[0] != 0 || k >= st[2]) return;
  const int n = st[1];
  double* D = ws + (size_t)bi * tstride + (size_t)k * FB * lw + (size_t)k * FB;
  const int t = threadIdx.x, c = t & 63, g = t >> 6;
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int r = g + 4 * e;
    A[r][c] = r <= c ? D[(size_t)r * lw + c] : 0.0;
  }
  __syncthreads();
  int bad = 0;
  double lsum = 0.0;                                   // (thread 0) sum of ln u_jj, in the order of j
  for (int j = 0; j < FB; ++j) {
    const double piv = A[j][j];
    if (!(piv > 0.0) || !(piv < __builtin_inf())) {    // (workgroup-uniform: every thread reads the same word)
      bad = j + 1;
      break;
    }
    const double d = sqrt(piv);
    if (t == 0 && k * FB + j < n) lsum += log(d);
    __syncthreads();                                   // every thread has read the pivot
    if (t < FB) A[j][t] = t == j ? d : (t > j ? A[j][t] / d : 0.0);
    __syncthreads();
    const double ujc = A[j][c];
#pragma unroll 4
    for (int e = 0; e < 16; ++e) {
      const int r = g + 4 * e;
      if (r > j && r <= c) A[r][c] = fma(-A[j][r], ujc, A[r][c]);
    }
    __syncthreads();
  }
  if (bad) {
    if (t == 0) {
      st[0] = k * FB + bad;
      flog[bi] = __builtin_nan("");
    }
    return;
  }
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int r = g + 4 * e;
    D[(size_t)r * lw + c] = r <= c ? A[r][c] : 0.0;
  }
  if (t == 0) flog[bi] += 2.0 * lsum;
}

// ---- the row panel of step k: X = U_kk^-T A(k, > k) ----
// grid (column groups of 256, count); thread = one column.
__global__ __launch_bounds__(256) void k_factor_panel(double* __restrict__ ws, size_t tstride, int lw, int k,
                                                      const int* __restrict__ fstat) {
  __shared__ double Lt[FB][FB + 1];                      // Lt[r][p] = U_kk[p][r]
  const int bi = blockIdx.y;
  const int* st = fstat + 4 * bi;
  const int nblk = st[2];
  if (st[0] != 0 || k + 1 >= nblk) return;
  const int t = threadIdx.x;
  const int c = (k + 1) * FB + blockIdx.x * 256 + t;
  if ((k + 1) * FB + (int)blockIdx.x * 256 >= nblk * FB) return;   // (workgroup-uniform)
  double* R = ws + (size_t)bi * tstride + (size_t)k * FB * lw;    // the block's rows
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int p = (t >> 6) + 4 * e;
    Lt[t & 63][p] = R[(size_t)p * lw + k * FB + (t & 63)];
  }
  __syncthreads();
  if (c >= nblk * FB) return;
  double x[FB];
#pragma unroll
  for (int r = 0; r < FB; ++r) x[r] = R[(size_t)r * lw + c];
#pragma unroll
  for (int r = 0; r < FB; ++r) {
    double s = x[r];
#pragma unroll
    for (int p = 0; p < r; ++p) s = fma(-Lt[r][p], x[p], s);
    x[r] = s / Lt[r][r];
  }
#pragma unroll
  for (int r = 0; r < FB; ++r) R[(size_t)r * lw + c] = x[r];
}

// ---- the trailing down-date of step k ----
// grid (tiles of the largest trailing triangle, count): tile x = (tr, tc), tr <= tc, of 128 x 128 from block k + 1 on.
__global__ __launch_bounds__(256) void k_factor_trail(double* __restrict__ ws, size_t tstride, int lw, int k, int t_hi,
                                                         const int* __restrict__ fstat) {
  __shared__ __attribute__((aligned(16))) double As[FT_KH][FT_LS];
  __shared__ __attribute__((aligned(16))) double Bs[FT_KH][FT_LS];
  const int bi = blockIdx.y;
  const int* st = fstat + 4 * bi;
  const int nblk = st[2], m = nblk - k - 1;            // trailing blocks of this trajectory
  if (st[0] != 0 || m <= 0) return;
  int tr = 0, rem = blockIdx.x;
  while (rem >= t_hi - tr) {
    rem -= t_hi - tr;
    ++tr;
  }
  const int tc = tr + rem;
  if (2 * tc >= m) return;                             // (tr <= tc: the tile's first block lies beyond the trajectory)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  const int br = 2 * tr + wr, bc = 2 * tc + wc;        // this wave's block of the trailing triangle
  const bool active = br < m && bc < m && br <= bc;
  double* A = ws + (size_t)bi * tstride;
  const int i0 = (k + 1) * FB + 128 * tr, j0 = (k + 1) * FB + 128 * tc, cend = nblk * FB;
  const double* Pk = A + (size_t)k * FB * lw;         // the panel: rows of block k

  double4_t acc[4][4];
  if (active) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[i][j][r] = A[(size_t)(i0 + wr * 64 + i * 16 + lk + 4 * r) * lw + j0 + wc * 64 + j * 16 + li];
  }
  // staging: thread (row tid >> 4 of the sixteen, 8 columns from (tid & 15) * 8) of either operand; columns beyond the
  // trajectory's blocks are zero (no wave that multiplies reads them)
  const int sr = tid >> 4, sc = (tid & 15) * 8;
  for (int half = 0; half < FB / FT_KH; ++half) {
    if (half) __syncthreads();
    const double* row = Pk + (size_t)(half * FT_KH + sr) * lw;
    const bool va = i0 + sc < cend, vb = j0 + sc < cend;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double2 a = make_double2(0.0, 0.0), b = make_double2(0.0, 0.0);
      if (va) a = *reinterpret_cast<const double2*>(row + i0 + sc + 2 * q);
      if (vb) b = *reinterpret_cast<const double2*>(row + j0 + sc + 2 * q);
      *reinterpret_cast<double2*>(&As[sr][sc + 2 * q]) = make_double2(-a.x, -a.y);   // the down-date's sign
      *reinterpret_cast<double2*>(&Bs[sr][sc + 2 * q]) = b;
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int kk = 0; kk < FT_KH / 4; ++kk) {
        double af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = As[4 * kk + lk][wr * 64 + i * 16 + li];
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = Bs[4 * kk + lk][wc * 64 + j * 16 + li];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          A[(size_t)(i0 + wr * 64 + i * 16 + lk + 4 * r) * lw + j0 + wc * 64 + j * 16 + li] = acc[i][j][r];
  }
}

// ---- block column bj of U against a vector's rows [row0, rows): acc[q] = sum_p U[p][64 bj + c] x[q][p] ----
// 256 threads = (column c = t & 63, row group g = t >> 6).  The rows go through LDS in chunks of 64, [row][rhs]; group g takes
// rows 16 g .. 16 g + 15 of every chunk, in ascending order; red[g][c][q] then holds the four partial sums, which the caller
// adds in the order of g.  Rows at or beyond n and right-hand sides at or beyond nrhs count as zero.
__device__ __forceinline__ void col_block_dot(const double* __restrict__ U, int lw, int bj, int row0, int rows, int n,
                                              const double* __restrict__ x, int nrhs, int stride, double (*xl)[FR],
                                              double (*red)[FB][FR + 1]) {
  const int t = threadIdx.x, c = t & 63, g = t >> 6;
  double acc[FR];
#pragma unroll
  for (int q = 0; q < FR; ++q) acc[q] = 0.0;
  for (int p0 = row0; p0 < rows; p0 += FB) {
    const double* Uc = U + (size_t)(p0 + 16 * g) * lw + bj * FB + c;
    double u[16];                                      // (all sixteen loads in flight before the chunk is staged)
#pragma unroll
    for (int s = 0; s < 16; ++s) u[s] = Uc[(size_t)s * lw];
    __syncthreads();
    for (int e = t; e < FB * FR; e += 256) {           // (e = q * 64 + row: consecutive threads read consecutive rows)
      const int q = e >> 6, p = p0 + (e & 63);
      xl[e & 63][q] = (q < nrhs && p < n) ? x[(size_t)q * stride + p] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
#pragma unroll
      for (int q = 0; q < FR; ++q) acc[q] = fma(u[s], xl[16 * g + s][q], acc[q]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < FR; ++q) red[g][c][q] = acc[q];
  __syncthreads();
}

// ---- white = U^-T rhs, quad = |white|^2: forward substitution with U^T, right-looking, two launches per block step bj ----
// x, white: [count][nrhs][stride]; quad: [count][nrhs]; trajectories [f0, f0 + count) of the factored range.  x starts as the
// right-hand sides and is updated in place: when step bj begins, its rows of block bj have lost the contributions of every
// row above.
// k_factor_solve_diag, one workgroup per trajectory: the block's 64 rows of white by substitution with the diagonal block
// (thread (c, g): row c of right-hand sides g, g + 4, g + 8, g + 12), their share of quad (added in the order of the rows), and
// at the trajectory's last block the NaN beyond n.  A failed trajectory is NaN throughout (written at step 0).
__global__ __launch_bounds__(256) void k_factor_solve_diag(const double* __restrict__ ws, size_t tstride, int lw,
                                                           const int* __restrict__ fstat, int f0, int bj, const double* __restrict__ x,
                                                           int nrhs, int stride, double* __restrict__ white, double* __restrict__ quad) {
  __shared__ double Ud[FB][FB + 1];
  __shared__ double wl[FB][FR];
  const int bi = blockIdx.x, t = threadIdx.x, c = t & 63, g = t >> 6;
  const int* st = fstat + 4 * (f0 + bi);
  const int n = st[1], nblk = st[2];
  const double nanv = __builtin_nan("");
  double* w = white + (size_t)bi * nrhs * stride;
  if (st[0] != 0) {
    if (bj == 0) {
      for (int e = t; e < nrhs * stride; e += 256) w[e] = nanv;
      if (t < nrhs) quad[(size_t)bi * nrhs + t] = nanv;
    }
    return;
  }
  if (bj >= nblk) return;
  const double* U = ws + (size_t)(f0 + bi) * tstride;
  const double* r = x + (size_t)bi * nrhs * stride;
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int p = g + 4 * e;
    Ud[p][c] = U[(size_t)(bj * FB + p) * lw + bj * FB + c];
  }
  double v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = g + 4 * e, row = bj * FB + c;
    v[e] = q < nrhs && row < n ? r[(size_t)q * stride + row] : 0.0;
  }
  __syncthreads();
  for (int j = 0; j < FB; ++j) {
    if (c == j) {
      const double d = Ud[j][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) wl[j][g + 4 * e] = v[e] / d;
    }
    __syncthreads();
    if (c > j) {
      const double u = Ud[j][c];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fma(-u, wl[j][g + 4 * e], v[e]);
    }
  }
  for (int e = t; e < FB * FR; e += 256) {             // (wl is complete: the last step's barrier)
    const int q = e >> 6, row = bj * FB + (e & 63);
    if (q < nrhs && row < n) w[(size_t)q * stride + row] = wl[e & 63][q];
  }
  if (t < nrhs) {
    double qsum = bj ? quad[(size_t)bi * nrhs + t] : 0.0;
    for (int j = 0; j < FB && bj * FB + j < n; ++j) qsum = fma(wl[j][t], wl[j][t], qsum);
    quad[(size_t)bi * nrhs + t] = qsum;
  }
  if (bj == nblk - 1)
    for (int q = 0; q < nrhs; ++q)
      for (int e = n + t; e < stride; e += 256) w[(size_t)q * stride + e] = nanv;
}
// k_factor_solve_update, grid (block columns to the right of bj, count): x(column block cb) -= U(bj, cb)^T white(bj)
__global__ __launch_bounds__(256) void k_factor_solve_update(const double* __restrict__ ws, size_t tstride, int lw,
                                                             const int* __restrict__ fstat, int f0, int bj,
                                                             const double* __restrict__ white, int nrhs, int stride,
                                                             double* __restrict__ x) {
  __shared__ double xl[FB][FR];
  __shared__ double red[4][FB][FR + 1];
  const int bi = blockIdx.y, cb = bj + 1 + blockIdx.x, t = threadIdx.x, c = t & 63, g = t >> 6;
  const int* st = fstat + 4 * (f0 + bi);
  const int n = st[1];
  if (st[0] != 0 || cb >= st[2]) return;
  col_block_dot(ws + (size_t)(f0 + bi) * tstride, lw, cb, bj * FB, (bj + 1) * FB, n, white + (size_t)bi * nrhs * stride, nrhs,
                stride, xl, red);
  double* r = x + (size_t)bi * nrhs * stride;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = g + 4 * e, col = cb * FB + c;
    const double s = ((red[0][c][q] + red[1][c][q]) + red[2][c][q]) + red[3][c][q];
    if (q < nrhs && col < n) r[(size_t)q * stride + col] -= s;
  }
}

// ---- out = U^T z; grid (nblk_hi, count): a workgroup per column block ----
__global__ __launch_bounds__(256) void k_factor_multiply(const double* __restrict__ ws, size_t tstride, int lw,
                                                         const int* __restrict__ fstat, int f0, const double* __restrict__ z,
                                                         int nrhs, int stride, double* __restrict__ out) {
  __shared__ double xl[FB][FR];
  __shared__ double red[4][FB][FR + 1];
  const int bi = blockIdx.y, bj = blockIdx.x, t = threadIdx.x, c = t & 63, g = t >> 6;
  const int* st = fstat + 4 * (f0 + bi);
  const int n = st[1], nblk = st[2];
  const double nanv = __builtin_nan("");
  double* o = out + (size_t)bi * nrhs * stride;
  if (st[0] != 0 || bj >= nblk) {
    // a failed trajectory is NaN throughout; beyond the trajectory's blocks: the tail up to stride
    for (int q = 0; q < nrhs; ++q) {
      const int col = bj * FB + t;
      if (t < FB && col < stride) o[(size_t)q * stride + col] = nanv;
    }
    return;
  }
  const double* U = ws + (size_t)(f0 + bi) * tstride;
  // (rows below the diagonal inside block bj are zero in the workspace, the padding rows meet zeroed entries of z)
  col_block_dot(U, lw, bj, 0, (bj + 1) * FB, n, z + (size_t)bi * nrhs * stride, nrhs, stride, xl, red);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = g + 4 * e, col = bj * FB + c;
    const double s = ((red[0][c][q] + red[1][c][q]) + red[2][c][q]) + red[3][c][q];
    if (q < nrhs && col < stride) o[(size_t)q * stride + col] = col < n ? s : nanv;
  }
}

// k_factor_multiply covers the columns below 64 * nblk_hi; what lies between that and stride (a caller's stride beyond the
// workspace's row stride) is NaN as well
__global__ void k_factor_tail(double* __restrict__ out, int count, int nrhs, int stride, int from) {
  const int width = stride - from;
  const long total = (long)count * nrhs * width;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    out[(e / width) * stride + from + (e % width)] = __builtin_nan("");
}

void launch_factor(hipStream_t st, const PendingView& f, const FactorView& w, int nblk_hi) {
  hipLaunchKernelGGL(k_factor_load, dim3(nblk_hi, nblk_hi, f.count), dim3(256), 0, st, f.P, f.nact, f.ld, f.pstride, f.b0, w.ws,
                     w.tstride, w.lw, w.fstat, w.flog);
  for (int k = 0; k < nblk_hi; ++k) {
    hipLaunchKernelGGL(k_factor_diag, dim3(f.count), dim3(256), 0, st, w.ws, w.tstride, w.lw, k, w.fstat, w.flog);
    if (k + 1 == nblk_hi) break;
    hipLaunchKernelGGL(k_factor_panel, dim3(factor_panel_groups(nblk_hi, k), f.count), dim3(256), 0, st, w.ws, w.tstride, w.lw, k,
                       w.fstat);
    const int t_hi = factor_trail_tiles_per_row(nblk_hi, k);
    hipLaunchKernelGGL(k_factor_trail, dim3(t_hi * (t_hi + 1) / 2, f.count), dim3(256), 0, st, w.ws, w.tstride, w.lw, k, t_hi,
                       w.fstat);
  }
}

void launch_factor_solve(hipStream_t st, const FactorView& w, int f0, int count, int nblk_hi, double* x, int nrhs, int stride,
                         double* white, double* quad) {
  for (int bj = 0; bj < nblk_hi; ++bj) {
    hipLaunchKernelGGL(k_factor_solve_diag, dim3(count), dim3(256), 0, st, w.ws, w.tstride, w.lw, w.fstat, f0, bj, x, nrhs, stride,
                       white, quad);
    if (bj + 1 < nblk_hi)
      hipLaunchKernelGGL(k_factor_solve_update, dim3(nblk_hi - bj - 1, count), dim3(256), 0, st, w.ws, w.tstride, w.lw, w.fstat, f0,
                         bj, white, nrhs, stride, x);
  }
}

void launch_factor_multiply(hipStream_t st, const FactorView& w, int f0, int count, int nblk_hi, const double* z, int nrhs,
                            int stride, double* out) {
  hipLaunchKernelGGL(k_factor_multiply, dim3(nblk_hi, count), dim3(256), 0, st, w.ws, w.tstride, w.lw, w.fstat, f0, z, nrhs,
                     stride, out);
  if (stride > nblk_hi * FB)
    hipLaunchKernelGGL(k_factor_tail, dim3(64), dim3(256), 0, st, out, count, nrhs, stride, nblk_hi * FB);
}

}  // namespace ekf
