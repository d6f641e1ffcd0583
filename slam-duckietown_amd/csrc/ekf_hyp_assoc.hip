// k_hyp_score: likelihood association of UNLABELLED range/bearing observations per hypothesis of a bank (ekf_hypotheses_associate,
// ekf_hypotheses_step_unlabelled, ekf_hypotheses_update_unlabelled; gfx950, wave64).  For hypothesis k, every landmark l of the
// bank's map (state indices i = 3 + 2 l, i + 1) and every observation q < m of ONE list shared by the hypotheses:
//     P5  = the joint covariance of (pose, landmark l): the pose block from st[k].blk, the cross terms X[r ldx + i], X[r ldx + i + 1]
//           of the hypothesis's rows (zero at and beyond its bound, as stored), the landmark block from the shared map;
//     m5  = st[k].pose and the map's mean of landmark l;
//     S, S^-1, ln det S, the innovation, NIS and the score d = NIS + ln det S: assoc_score (ekf_assoc_score.h), the function
//           k_assoc_query calls -- the same p5 / m5 / noise pair / observations give the same bits as ekf_associate on a slot that
//           adopted the hypothesis (recorded once in profiles/hyp_associate.txt: the move left ekf_associate's bits alone);
// and per observation the two smallest scores with their landmark, NIS and ln det S, plus the smallest NIS of all, by
// AssocBest::offer: a strictly smaller score replaces, ties stay with the lower landmark, a NaN never wins, an empty map or
// all-NaN scores give -1 / NaN.  A hypothesis's result depends on its own state, the map and the observations -- not on K, on k
// or on which hypotheses share the launch.
//
// Shape (plan_hyp_associate, ekf_host_plan.h): ONE workgroup of 4 waves per hypothesis of the range, lane = landmark within a chunk
// of 64.  Wave w walks the CONTIGUOUS ascending chunks [w cpw, (w + 1) cpw), cpw = ceil(chunks / 4); a chunk's 64 x (m + 1) numbers
// (NIS per observation, ln det S) go through the wave's LDS, lane q then scans observation q's 64 scores in ascending landmark order
// into its running two best, kept in registers across the wave's chunks.  The four waves' records are merged by wave 0 in wave
// order -- ascending landmark order -- by the same offer: the reduction order is fixed and no second kernel is needed.  The kernel
// reads a hypothesis's three rows once (24 n bytes); the 2 x 2 landmark blocks and means are the same ~5 n doubles for every
// hypothesis and stay in L2.
//
// Two modes, the same scores in both.  QUERY (o.cand): the per-hypothesis results to device buffers shaped as ekf_associate's with
// stride = m.  STEP (o.step): wave 0 also resolves the assignment -- frontend.resolve_associations with no new landmarks: the
// observations in ascending order of their best candidate's NIS (stable, NaN last), each takes its first candidate of two that
// no earlier one took and is accepted iff that candidate's NIS <= accept, else dropped -- and writes hypothesis k's StepIn (the
// accepted pairs in observation order; flags, m, neff and padding as ekf_hyp_update's packing writes them for that list), its
// assignment row, and adds dropped * miss to st[k].loglik (one product, one addition; only where dropped > 0 and miss != 0).
// The query writes nothing of the bank; the step mode writes loglik alone.
#include <cmath>

#include "ekf_device.h"

#include "ekf_assoc_score.h"
#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

static_assert(HS_CHUNK == 64, "lane = landmark: a chunk is one wave of landmarks");

__global__ __launch_bounds__(64 * HS_WAVES) void k_hyp_score(const double* __restrict__ Pm, const double* __restrict__ mum,
                                                             HypState* __restrict__ st, const double* __restrict__ X,
                                                             const DeviceConfig cfg, int n, int ld, int ldx, int k0, int chunks,
                                                             const double* __restrict__ zr, const double* __restrict__ zb, int m,
                                                             const HypScoreOut o) {
  __shared__ double sn[HS_WAVES][64][MMAX + 1], sl[HS_WAVES][64];
  __shared__ double wrec[HS_WAVES][MMAX][AQ_PART];
  __shared__ double f_nis[2][MMAX];
  __shared__ int f_lm[2][MMAX], s_ord[MMAX], s_asg[MMAX], s_cnt;
  const int bi = blockIdx.x, k = k0 + bi;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nl = (n - 3) >> 1;
  const double nanv = __builtin_nan("");
  const HypState& hs = st[k];
  const double* Xk = X + (long)k * 3 * ldx;
  double p5[5][5], m5[5];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    m5[a] = hs.pose[a];
#pragma unroll
    for (int c = a; c < 3; ++c) p5[a][c] = p5[c][a] = hs.blk[hyp_blk(a, c)];
  }
  const int cpw = (chunks + HS_WAVES - 1) / HS_WAVES;
  const int c0 = min(chunks, wave * cpw), c1 = min(chunks, c0 + cpw);
  AssocBest best;
  best.clear();
  double mn = nanv;
  for (int ch = c0; ch < c1; ++ch) {                     // (wave-uniform)
    const int l0 = ch * HS_CHUNK, l = l0 + lane;
    double nis_q[MMAX], logdet = nanv;
#pragma unroll
    for (int q = 0; q < MMAX; ++q) nis_q[q] = nanv;
    if (l < nl) {
      const int i = 3 + 2 * l;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        p5[a][3] = p5[3][a] = Xk[(long)a * ldx + i];
        p5[a][4] = p5[4][a] = Xk[(long)a * ldx + i + 1];
      }
      p5[3][3] = Pm[p_index(ld, i, i)];
      p5[3][4] = p5[4][3] = Pm[p_index(ld, i, i + 1)];
      p5[4][4] = Pm[p_index(ld, i + 1, i + 1)];
      m5[3] = mum[i];
      m5[4] = mum[i + 1];
      assoc_score(p5, m5, cfg.qd, zr, zb, m, nis_q, logdet);
    }
    sl[wave][lane] = logdet;
#pragma unroll
    for (int q = 0; q < MMAX; ++q) {
      sn[wave][lane][q] = nis_q[q];
      if (o.all_nis && l < o.cap && q < m) {
        o.all_nis[((long)bi * m + q) * o.cap + l] = nis_q[q];
        o.all_logdet[((long)bi * m + q) * o.cap + l] = logdet;
      }
    }
    WAVE_SYNC();
    // ---- lane q: observation q over the chunk's landmarks, ascending ----
    if (lane < m)
      for (int j = 0; j < HS_CHUNK; ++j) {
        const double nv = sn[wave][j][lane], lv = sl[wave][j];
        best.offer(nv + lv, (double)(l0 + j), nv, lv);
        mn = nan_min(mn, nv);
      }
    WAVE_SYNC();                                         // (the next chunk overwrites the wave's LDS)
  }
  if (lane < MMAX) {
    double* r = wrec[wave][lane];
    r[0] = best.d[0]; r[1] = best.lm[0]; r[2] = best.nis[0]; r[3] = best.ld[0];
    r[4] = best.d[1]; r[5] = best.lm[1]; r[6] = best.nis[1]; r[7] = best.ld[1];
    r[8] = mn;
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- wave 0, lane q: the four waves' records in wave order ----
  best.clear();
  mn = nanv;
  if (lane < m)
    for (int w = 0; w < HS_WAVES; ++w) {
      const double* r = wrec[w][lane];
      best.offer(r[0], r[1], r[2], r[3]);
      best.offer(r[4], r[5], r[6], r[7]);
      mn = nan_min(mn, r[8]);
    }
  if (o.cand) {
    if (lane < m) {
      const long q = (long)bi * m + lane;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        o.cand[2 * q + e] = (int)best.lm[e];
        if (o.cand_nis) o.cand_nis[2 * q + e] = best.nis[e];
        if (o.cand_logdet) o.cand_logdet[2 * q + e] = best.ld[e];
      }
      if (o.min_nis) o.min_nis[q] = mn;
    }
    return;
  }

  // ---- step mode: the assignment, the record, the clutter term ----
  if (lane < MMAX) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      f_lm[e][lane] = lane < m ? (int)best.lm[e] : -1;
      f_nis[e][lane] = lane < m ? best.nis[e] : nanv;
    }
    s_asg[lane] = -1;
  }
  WAVE_SYNC();
  if (lane == 0) {
    // the observations by ascending NIS of their best candidate: stable insertion, NaN last (np.argsort(kind="stable"))
    for (int q = 0; q < m; ++q) {
      const double v = f_nis[0][q];
      int p = q;
      while (p > 0) {
        const double u = f_nis[0][s_ord[p - 1]];
        if (!(v < u || (v == v && !(u == u)))) break;    // (u stays in front unless v is strictly smaller, or u is NaN and v is not)
        s_ord[p] = s_ord[p - 1];
        --p;
      }
      s_ord[p] = q;
    }
    int cnt = 0;
    for (int t = 0; t < m; ++t) {
      const int q = s_ord[t];
      int pick = -1;
      for (int e = 0; e < 2 && pick < 0; ++e) {
        const int c = f_lm[e][q];
        if (c < 0) continue;
        bool taken = false;
        for (int u = 0; u < t; ++u) taken = taken || s_asg[s_ord[u]] == c;
        if (!taken) pick = e;
      }
      if (pick >= 0 && f_nis[pick][q] <= o.accept) {     // (NaN compares false: dropped)
        s_asg[q] = f_lm[pick][q];
        cnt += 1;
      }
    }
    s_cnt = cnt;
    const int dropped = m - cnt;
    if (dropped > 0 && o.miss != 0.0) st[k].loglik = __dadd_rn(st[k].loglik, __dmul_rn((double)dropped, o.miss));
  }
  WAVE_SYNC();
  StepIn& s = o.step[k];
  const int cnt = s_cnt;
  const int mine = lane < MMAX ? s_asg[lane] : -1;
  const unsigned long long acc = __ballot(mine >= 0);
  if (lane < MMAX) {
    o.assign[(long)k * MMAX + lane] = mine;
    if (mine >= 0) {                                     // the accepted pairs in observation order
      const int p = __popcll(acc & ((1ull << lane) - 1ull));
      s.idx[p] = mine;
      s.range[p] = zr[lane];
      s.bearing[p] = zb[lane];
    }
    if (lane >= cnt) {
      s.idx[lane] = 0;
      s.range[lane] = 0.0;
      s.bearing[lane] = 0.0;
    }
  }
  if (lane == 0) {
    int bound = 3;                                       // fill_step's StepIn::neff for this list (the bank's solve does not read it)
    for (int q = 0; q < m; ++q)
      if (s_asg[q] >= 0) bound = max(bound, 3 + 2 * (s_asg[q] + 1));
    s.lin = 0.0;
    s.ang = 0.0;
    s.m = cnt;
    s.flags = FLAG_UPDATE;
    s.neff = min(bound, n);
    s.pad = 0;
  }
}

void launch_hyp_score(hipStream_t st, const HypView& v, const DeviceConfig& cfg, int k0, int count, int chunks, const double* zr,
                      const double* zb, int m, const HypScoreOut& o) {
  hipLaunchKernelGGL(k_hyp_score, dim3(count), dim3(64 * HS_WAVES), 0, st, v.map, v.mu, v.st, v.X, cfg, v.n, v.ld, v.ldx, k0, chunks,
                     zr, zb, m, o);
}

}  // namespace ekf
