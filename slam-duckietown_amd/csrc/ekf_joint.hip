// k_joint: the CURRENT joint covariance (and mean) of the pose and a chosen subset of landmarks, without applying the pending
// update (ekf_download_joint; gfx950, wave64).  Every entry is read as k_marginals (ekf_marginals.hip) reads its blocks:
//     P(a, c) = P_base[a][c] + sum_k W[a][k] V[k][c] + [a == c < 3] dacc[a]      (a <= c, state indices)
// over the kb pending ranks (the count rounded up to a k-tile), the ranks only where c lies below min(nact[b], so[b].neff),
// nothing added at all -- neither ranks nor dacc -- when kb == 0 (P_base bit for bit).  Read-only: nothing the filter owns is
// written.  Layouts: P_base through p_index (column panels beyond ld = 4096), V rank-major with row stride ld, W in MFMA A tiles
// (wm_index).
//
// The host hands over each trajectory's sub-state SORTED by state index (plan_joint_query / ekf_download_joint): `sidx` the
// state index of sorted entry t, `spos` the row / column of the output it belongs to; entries beyond the trajectory's own
// 3 + 2 k are sidx = -1 (their rows and columns are NaN), entries beyond ns -- the padding to whole tiles -- spos = -1
// (nothing is written).  In sorted order the stored upper triangle of P is the upper triangle of the sub-matrix, so:
//
// Shape: workgroup (x, bi) = 4 waves on one JQ_TILE x JQ_TILE tile (tr <= tc) of the sorted sub-matrix of trajectory b0 + bi.
// It stages the W rows of the tile's 32 row indices and the V columns of its 32 column indices over the kb ranks once in LDS
// (2 x 20 KB: W as [row][rank] with a row pad -- a half-wave reads one row, a broadcast --, V as [rank][column] -- a half-wave
// reads 32 consecutive doubles, one bank row), then thread (c = t & 31, r = t >> 5 + 8 e, e < 4) forms its four entries: one
// chain of FMAs over the ranks in ascending order, whatever the selection -- a permuted selection permutes the result and a
// subset returns the superset's entries bit for bit --, added to the base entry, written at (spos r, spos c) and mirrored.  Of a
// diagonal tile only r <= c is formed.  Its first half-wave also writes the tile's part of the mean.
#include <cmath>

#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int JQ_THREADS = 256;
constexpr int JQ_WPAD = KTOT + 1;        // doubles per staged W row: rows 2 (mod 32) banks apart for the staging stores
static_assert(JQ_TILE == 32 && JQ_THREADS == 8 * JQ_TILE, "thread = (column, row mod 8) of a 32 x 32 tile");

__global__ __launch_bounds__(JQ_THREADS) void k_joint(const double* __restrict__ P, const double* __restrict__ V,
                                                      const double* __restrict__ W, const double* __restrict__ dacc,
                                                      const double* __restrict__ mu, const int* __restrict__ nact,
                                                      const SolveOut* __restrict__ so, int ld, long pstride, int b0, int kb,
                                                      int ns, int nt, const int* __restrict__ sel,
                                                      double* __restrict__ mean_out, double* __restrict__ cov_out) {
  __shared__ double Wl[JQ_TILE][JQ_WPAD];
  __shared__ double Vl[KTOT][JQ_TILE];
  const int bi = blockIdx.y, b = b0 + bi;
  int tr = 0, rem = blockIdx.x;                        // tile x of the upper triangle, row-major: (tr, tc), tr <= tc < nt
  while (rem >= nt - tr) {
    rem -= nt - tr;
    ++tr;
  }
  const int tc = tr + rem;
  const int nsp = nt * JQ_TILE;
  const int* sidx = sel + (long)bi * 2 * nsp;
  const int* spos = sidx + nsp;
  const int t = threadIdx.x, c = t & (JQ_TILE - 1), rq = t >> 5;
  const int n = nact[b];
  const int bound = kb > 0 ? min(n, so[b].neff) : 0;   // state indices below it take the pending ranks
  const double* Pb = P + (long)b * pstride;
  const double nanv = __builtin_nan("");

  const int ic = sidx[tc * JQ_TILE + c], pc = spos[tc * JQ_TILE + c];
  // the base entries first: their latency hides under the staging
  int ir[4], pr[4];
  double base[4];
  bool own[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = rq + 8 * e;
    ir[e] = sidx[tr * JQ_TILE + r];
    pr[e] = spos[tr * JQ_TILE + r];
    own[e] = pr[e] >= 0 && pc >= 0 && (tr < tc || r <= c);
    base[e] = (own[e] && ir[e] >= 0 && ic >= 0) ? Pb[p_index(ld, ir[e], ic)] : nanv;   // (sorted: ir <= ic)
  }

  // ---- the mean of the tile's entries (diagonal tiles) ----
  if (mean_out && tr == tc && t < JQ_TILE && pc >= 0)
    mean_out[(long)bi * ns + pc] = ic >= 0 ? mu[(long)b * ld + ic] : nanv;

  // ---- the ranks: stage, then one chain per entry ----
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const int first = sidx[tc * JQ_TILE];                // the tile's smallest column index (sorted; -1: no column at all)
  if (first >= 0 && first < bound) {                   // (workgroup-uniform; bound == 0 without pending ranks)
    const __amdgpu_buffer_rsrc_t rsV = rs_rsrc(V + (long)b * KTOT * ld), rsW = rs_rsrc(W + (long)b * KTOT * ld);
    const int ld16 = ld >> 4;
    const int iw = sidx[tr * JQ_TILE + c];             // this thread stages row c of W and column c of V, the ranks rq, rq + 8, ..
    const unsigned wi = iw >= 0 ? (unsigned)((iw >> 4) * 64 + (iw & 15)) * 8u : 0u;
    const unsigned vi = ic >= 0 ? (unsigned)ic * 8u : 0u, vrow = (unsigned)ld * 8u;
    for (int k = rq; k < kb; k += 8) {
      const unsigned kw = (unsigned)(((k >> 2) * ld16) * 64 + (k & 3) * 16) * 8u;   // wm_index: rank part
      // (k differs between the two halves of a wave: the rank part goes into the per-lane offset, the scalar one stays zero)
      const double w = ldb8(rsW, wi + kw, 0u), v = ldb8(rsV, vi + (unsigned)k * vrow, 0u);
      Wl[c][k] = iw >= 0 ? w : 0.0;
      Vl[k][c] = ic >= 0 ? v : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < kb; k += 4) {                  // (kb is a multiple of 4)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double v = Vl[k + kk][c];
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = fma(Wl[rq + 8 * e][k + kk], v, s[e]);
      }
    }
  }

#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!own[e]) continue;
    double v = base[e];
    if (ir[e] >= 0 && ic >= 0) {
      if (ic < bound) v += s[e];
      if (kb > 0 && ir[e] == ic && ic < 3) v += dacc[4 * b + ic];
    }
    double* o = cov_out + (long)bi * ns * ns;
    o[(long)pr[e] * ns + pc] = v;
    if (pr[e] != pc) o[(long)pc * ns + pr[e]] = v;     // the mirrored entry, by whoever formed the upper one
  }
}

void launch_joint(hipStream_t st, const PendingView& f, int ns, int nt, int tiles, const int* sel, double* mean_out,
                  double* cov_out) {
  hipLaunchKernelGGL(k_joint, dim3(tiles, f.count), dim3(JQ_THREADS), 0, st, f.P, f.V, f.W, f.dacc, f.mu, f.nact, f.so, f.ld,
                     f.pstride, f.b0, f.kb, ns, nt, sel, mean_out, cov_out);
}

}  // namespace ekf
