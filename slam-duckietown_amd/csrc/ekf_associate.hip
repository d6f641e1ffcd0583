// k_assoc_query / k_assoc_finish: likelihood association of unlabelled range/bearing observations (ekf_associate; gfx950,
// wave64).  For trajectory b, every landmark l of its map (state indices i = 3 + 2 l, i + 1) and every observation q < m[b]:
//     P5  = the CURRENT joint covariance of (pose, landmark l), 5 x 5, read as k_marginals (ekf_marginals.hip) reads its blocks:
//           P(a, c) = P_base[a][c] + sum_k W[a][k] V[k][c] + [a == c < 3] dacc[a]     (a <= c)
//           over the kb pending ranks, the ranks only where the column index c lies below min(nact[b], so[b].neff), nothing
//           added at all -- neither ranks nor dacc -- when kb == 0 (P_base bit for bit);
//     d, q, z^ and the 2 x 5 Jacobian H5 of the measurement model at the current mean (src/replay_no_ros.py:443-469);
//     S   = H5 P5 H5^T + Q_b, S^-1, ln det S                                            (once per landmark)
//     y   = z_q - z^, bearing wrapped; NIS = y^T S^-1 y; score d = NIS + ln det S      (per observation)
// and per observation the two smallest scores with their landmark, NIS and ln det S, plus the smallest NIS of all.
// Read-only: nothing the filter owns is written.
//
// Shape: k_marginals' -- workgroup (x, bi) = 4 waves over the 64 landmarks 64 x .. 64 x + 63 of trajectory b0 + bi, lane =
// landmark; the four waves split the k-tiles of the pending ranks (the V loads are the marginal's; the three pose rows of W are
// staged once per workgroup in LDS and cost six more FMAs per rank), wave 1 forms the pose block (lane = rank), wave 0 adds the
// partial sums in a fixed order, linearises, scores and reduces.
// The reduction is deterministic, in two stages with no atomics: lane q of wave 0 scans the workgroup's 64 scores of
// observation q in ascending landmark order (a strictly smaller score replaces: ties stay with the lower index; a NaN never
// wins) and leaves one partial record per (trajectory, chunk, observation); k_assoc_finish merges a trajectory's records in
// ascending chunk order the same way.  A trajectory without landmarks, or whose scores are all NaN, ends with index -1 and NaN.
#include <cmath>

#include "ekf_device.h"

#include "ekf_assoc_score.h"
#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

constexpr int AQ_WAVES = 4;
static_assert(AQ_CHUNK == 64, "lane = landmark: a chunk is one wave of landmarks");
constexpr int AQ_SUMS = 9;              // per lane: the landmark block (3) and the 3 x 2 cross block (6) over the ranks

struct AssocTile {
  double v0[4], v1[4], w0[4], w1[4];    // V[k][i], V[k][i + 1], W[i][k], W[i + 1][k] for the 4 ranks of a k-tile
};
// (the scoring arithmetic, AssocBest and nan_min: ekf_assoc_score.h, shared with k_hyp_score)

__global__ __launch_bounds__(64 * AQ_WAVES) void k_assoc_query(
    const double* __restrict__ P, const double* __restrict__ V, const double* __restrict__ W, const double* __restrict__ dacc,
    const double* __restrict__ mu, const int* __restrict__ nact, const SolveOut* __restrict__ so, const DeviceConfig cfg, int ld,
    long pstride, int b0, int kb, int stride, int cap, const double* __restrict__ zr, const double* __restrict__ zb,
    const int* __restrict__ zm, double* __restrict__ part_out, double* __restrict__ all_nis, double* __restrict__ all_logdet) {
  __shared__ double part[AQ_WAVES][AQ_SUMS][64];
  __shared__ double wp[3][KTOT];                       // W[a][k], a < 3: uniform per trajectory
  __shared__ double pose_s[9];
  __shared__ double sd[64][MMAX + 1], sn[64][MMAX + 1], sl[64];
  const int bi = blockIdx.y, b = b0 + bi;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = nact[b];
  const int nl = (n - 3) >> 1;
  const int bound = kb > 0 ? min(n, so[b].neff) : 0;   // state indices below it take the pending ranks
  const int mb = zm[bi];
  const double nanv = __builtin_nan("");
  const int l0 = blockIdx.x * AQ_CHUNK;                // first landmark of the workgroup
  const int l = l0 + lane;
  double* rec = part_out + (((long)bi * gridDim.x + blockIdx.x) * stride) * AQ_PART;
  if (l0 >= nl) {                                      // (workgroup-uniform) no landmark here: NaN rows, an empty record
    if (wave == 0) {
      if (all_nis && l < cap)
        for (int q = 0; q < stride; ++q) {
          all_nis[((long)bi * stride + q) * cap + l] = nanv;
          all_logdet[((long)bi * stride + q) * cap + l] = nanv;
        }
      if (lane < stride) {
        double* r = rec + lane * AQ_PART;
#pragma unroll
        for (int e = 0; e < AQ_PART; ++e) r[e] = (e == 1 || e == 5) ? -1.0 : nanv;
      }
    }
    return;
  }
  const double* Pb = P + (long)b * pstride;
  const double* Vb = V + (long)b * KTOT * ld;
  const double* Wb = W + (long)b * KTOT * ld;
  const double* mub = mu + (long)b * ld;
  const __amdgpu_buffer_rsrc_t rsV = rs_rsrc(Vb), rsW = rs_rsrc(Wb);
  const int ld16 = ld >> 4;
  const bool live = l < nl;
  const int i = live ? 3 + 2 * l : 3;                  // (lanes beyond the landmarks read landmark 0's entries, discarded)

  // ---- the three pose rows of W, once per workgroup ----
  double wrow[3] = {0.0, 0.0, 0.0};
  const int kt = (int)threadIdx.x;
  if (kt < kb) {
    const unsigned kw = (unsigned)(((kt >> 2) * ld16) * 64 + (kt & 3) * 16) * 8u;   // wm_index(ld16, k, 0)
    wrow[0] = ldb8(rsW, kw, 0u);
    wrow[1] = ldb8(rsW, kw, 8u);
    wrow[2] = ldb8(rsW, kw, 16u);
  }
  double base00 = 0.0, base01 = 0.0, base11 = 0.0, basec[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
  double m5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (wave == 0) {                                     // the base entries and the mean: their latency hides under the ranks
    base00 = Pb[p_index(ld, i, i)];
    base01 = Pb[p_index(ld, i, i + 1)];
    base11 = Pb[p_index(ld, i + 1, i + 1)];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      basec[a][0] = Pb[p_index(ld, a, i)];
      basec[a][1] = Pb[p_index(ld, a, i + 1)];
      m5[a] = mub[a];
    }
    m5[3] = mub[i];
    m5[4] = mub[i + 1];
  }
  const int nkt = kb >> 2;
  const bool ranks = 3 + 2 * l0 < bound && wave < nkt;   // (wave-uniform) a landmark below the bound, and this wave has a k-tile
  const unsigned vi = (unsigned)i * 8u, vrow = (unsigned)ld * 8u;
  const unsigned wi0 = (unsigned)((i >> 4) * 64 + (i & 15)) * 8u;
  const unsigned wi1 = (unsigned)(((i + 1) >> 4) * 64 + ((i + 1) & 15)) * 8u;
  auto load = [&](AssocTile& T, int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * t + r;
      T.v0[r] = ldb8(rsV, vi, (unsigned)k * vrow);
      T.v1[r] = ldb8(rsV, vi + 8u, (unsigned)k * vrow);
      const unsigned kw = (unsigned)((t * ld16) * 64 + r * 16) * 8u;   // wm_index: rank part (k-tile t, k & 3 = r)
      T.w0[r] = ldb8(rsW, wi0, kw);
      T.w1[r] = ldb8(rsW, wi1, kw);
    }
  };
  AssocTile A, B;
  if (ranks) load(A, wave);
  if (kt < kb) {
    wp[0][kt] = wrow[0];
    wp[1][kt] = wrow[1];
    wp[2][kt] = wrow[2];
  }
  __syncthreads();

  // ---- pose block (wave 1, lane = rank: k_marginals' sums, order and butterfly) ----
  if (wave == 1) {
    double s[6];                                       // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
#pragma unroll
    for (int e = 0; e < 6; ++e) s[e] = 0.0;
    for (int k0 = 0; k0 < kb; k0 += 64) {              // (kb <= 80: two rounds at most)
      const int k = k0 + lane;
      if (k < kb) {
        const unsigned kv = (unsigned)(k * ld) * 8u;
        const double v0 = ldb8(rsV, kv, 0u), v1 = ldb8(rsV, kv, 8u), v2 = ldb8(rsV, kv, 16u);
        const double w0 = wp[0][k], w1 = wp[1][k], w2 = wp[2][k];
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
    if (lane < 9) {                                    // lane = row-major entry of the 3 x 3 block, from its upper triangle
      const int r = lane / 3, c = lane - 3 * r;
      const int a = min(r, c), bb = max(r, c);
      double sum = 0.0;
      if (a == 0) sum = bb == 0 ? s[0] : (bb == 1 ? s[1] : s[2]);
      else if (a == 1) sum = bb == 1 ? s[3] : s[4];
      else sum = s[5];
      double v = Pb[p_index(ld, a, bb)];
      if (kb > 0) {                                    // (the pose indices always lie below the bound)
        v += sum;
        if (a == bb) v += dacc[4 * b + a];
      }
      pose_s[lane] = v;
    }
  }

  // ---- landmark block and cross block over the ranks ----
  double s00 = 0.0, s01 = 0.0, s11 = 0.0, sc[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
  if (ranks) {
    auto sum = [&](const AssocTile& T, int t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 4 * t + r;
        s00 = fma(T.w0[r], T.v0[r], s00);
        s01 = fma(T.w0[r], T.v1[r], s01);
        s11 = fma(T.w1[r], T.v1[r], s11);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double wa = wp[a][k];
          sc[a][0] = fma(wa, T.v0[r], sc[a][0]);
          sc[a][1] = fma(wa, T.v1[r], sc[a][1]);
        }
      }
    };
    int t = wave;
    for (;;) {
      const int tn = t + AQ_WAVES;
      if (tn < nkt) load(B, tn);                       // (wave-uniform) the next tile in flight while this one is summed
      sum(A, t);
      if (tn >= nkt) break;
      t = tn;
      const int tn2 = t + AQ_WAVES;
      if (tn2 < nkt) load(A, tn2);
      sum(B, t);
      if (tn2 >= nkt) break;
      t = tn2;
    }
  }
  part[wave][0][lane] = s00;
  part[wave][1][lane] = s01;
  part[wave][2][lane] = s11;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    part[wave][3 + 2 * a][lane] = sc[a][0];
    part[wave][4 + 2 * a][lane] = sc[a][1];
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- wave 0: the 5 x 5 block, the linearisation, S, the scores ----
  double nis_q[MMAX], logdet = nanv;
#pragma unroll
  for (int q = 0; q < MMAX; ++q) nis_q[q] = nanv;
  if (live) {
    double r[AQ_SUMS];
#pragma unroll
    for (int e = 0; e < AQ_SUMS; ++e) {
      r[e] = part[0][e][lane];
#pragma unroll
      for (int w = 1; w < AQ_WAVES; ++w) r[e] += part[w][e][lane];
    }
    double p5[5][5];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) p5[a][c] = pose_s[3 * a + c];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p5[a][3] = p5[3][a] = i < bound ? basec[a][0] + r[3 + 2 * a] : basec[a][0];
      p5[a][4] = p5[4][a] = i + 1 < bound ? basec[a][1] + r[4 + 2 * a] : basec[a][1];
    }
    p5[3][3] = i < bound ? base00 + r[0] : base00;
    p5[3][4] = p5[4][3] = i + 1 < bound ? base01 + r[1] : base01;
    p5[4][4] = i + 1 < bound ? base11 + r[2] : base11;
    const double* qd = cfg.noise ? cfg.noise + (long)NOISE_ROW * b + 3 : cfg.qd;   // Q_b (ekf_set_noise's row if the table is set)
    assoc_score(p5, m5, qd, zr + bi * stride, zb + bi * stride, mb, nis_q, logdet);   // (ekf_assoc_score.h)
  }
  sl[lane] = logdet;
#pragma unroll
  for (int q = 0; q < MMAX; ++q) {
    sn[lane][q] = nis_q[q];
    sd[lane][q] = nis_q[q] + logdet;
    if (all_nis && l < cap && q < stride) {
      all_nis[((long)bi * stride + q) * cap + l] = nis_q[q];
      all_logdet[((long)bi * stride + q) * cap + l] = q < mb ? logdet : nanv;
    }
  }
  WAVE_SYNC();
  // ---- lane q: observation q over the workgroup's landmarks, ascending ----
  if (lane < stride) {
    AssocBest best;
    best.clear();
    double mn = nanv;
    if (lane < mb)
      for (int j = 0; j < AQ_CHUNK; ++j) {
        best.offer(sd[j][lane], (double)(l0 + j), sn[j][lane], sl[j]);
        mn = nan_min(mn, sn[j][lane]);
      }
    double* r = rec + lane * AQ_PART;
    r[0] = best.d[0]; r[1] = best.lm[0]; r[2] = best.nis[0]; r[3] = best.ld[0];
    r[4] = best.d[1]; r[5] = best.lm[1]; r[6] = best.nis[1]; r[7] = best.ld[1];
    r[8] = mn;
  }
}

// One workgroup per trajectory, lane q = observation q: the chunks' records in ascending order.
__global__ __launch_bounds__(64) void k_assoc_finish(const double* __restrict__ part, int chunks, int stride,
                                                     const int* __restrict__ zm, int* __restrict__ cand,
                                                     double* __restrict__ cand_nis, double* __restrict__ cand_logdet,
                                                     double* __restrict__ min_nis) {
  const int bi = blockIdx.x, q = threadIdx.x;
  if (q >= stride) return;
  AssocBest best;
  best.clear();
  double mn = __builtin_nan("");
  if (q < zm[bi])
    for (int c = 0; c < chunks; ++c) {
      const double* r = part + (((long)bi * chunks + c) * stride + q) * AQ_PART;
      best.offer(r[0], r[1], r[2], r[3]);
      best.offer(r[4], r[5], r[6], r[7]);
      mn = nan_min(mn, r[8]);
    }
  const long o = (long)bi * stride + q;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    cand[2 * o + e] = (int)best.lm[e];
    if (cand_nis) cand_nis[2 * o + e] = best.nis[e];
    if (cand_logdet) cand_logdet[2 * o + e] = best.ld[e];
  }
  if (min_nis) min_nis[o] = mn;
}

long assoc_query_part_doubles(int count, int chunks, int stride) { return (long)count * chunks * stride * AQ_PART; }

void launch_assoc_query(hipStream_t st, const PendingView& f, const DeviceConfig& cfg, int stride, int cap, int chunks,
                        const double* zr, const double* zb, const int* zm, double* part, double* all_nis, double* all_logdet,
                        int* cand, double* cand_nis, double* cand_logdet, double* min_nis) {
  hipLaunchKernelGGL(k_assoc_query, dim3(chunks, f.count), dim3(64 * AQ_WAVES), 0, st, f.P, f.V, f.W, f.dacc, f.mu, f.nact, f.so,
                     cfg, f.ld, f.pstride, f.b0, f.kb, stride, cap, zr, zb, zm, part, all_nis, all_logdet);
  hipLaunchKernelGGL(k_assoc_finish, dim3(f.count), dim3(64), 0, st, part, chunks, stride, zm, cand, cand_nis, cand_logdet,
                     min_nis);
}

}  // namespace ekf
