// k_loc_associate: the device-side front end of ekf_localize_detections (gfx950, wave64) -- one window of raw AprilTag detections
// per trajectory turned into the StepIn records k_loc_solve (ekf_localize.hip) consumes, against a FROZEN map: tag-table lookup,
// IGNORE_TAGS, the 1.5 m gate, per-tag averaging, range and bearing (src/replay_no_ros.py:280-337), and nothing of :341-360 --
// no landmark is ever added.  One workgroup of ONE wave per trajectory, grid = batch.
// The walk is a COPY of k_associate's (ekf_kernels.hip; that kernel's bits are pinned all over the suite and it is not touched,
// as loc_motion is a copy of the step kernels' motion model): the same DetIn records, chunks of 64 detections, the ignore list,
// t2^2 + t0^2 > gate2, ids outside [0, TAGMAX) set EKF_FLAG_ASSOC, one slot per distinct tag in order of first appearance, sums
// then a division by the count, xr = t2, yr = -t0, sqrt, atan2, the world guess from the pose BEFORE the prediction -- in that
// order, without contraction, so a tag's averaged (range, bearing) has the bits k_associate would give it.
// What differs: a tag the table does not know, or whose entry points at or beyond the trajectory's landmark count (a stale row),
// is UNMATCHED -- no slot, no flag, nothing changes; its id goes to the trajectory's LocUnmatched record, distinct ids in order of
// first appearance (the first AMAX of them; `total` counts all).  More than AMAX distinct MATCHED tags: the surplus is dropped
// with EKF_FLAG_ASSOC, as in mapping.  Which ids were already seen as unmatched is a 1024-bit set held in registers (lane l < 32
// holds ids 32 l .. 32 l + 31), the list itself one id per lane: the walk's only LDS traffic stays k_associate's.
// Written: step_out[b] (FLAG_PREDICT | FLAG_UPDATE, up to MMAX observations) and step_out[batch + b] (the update-only rest),
// assoc_out[b] (the matched tags, n_after = n), unmatched[b], neff_dev[b] (raised over the matched landmarks, capped at n: a
// consider update correlates the pose with every landmark it names, and only the device knows which those are), the sticky flag.
// NOT written: tagmap, nact, P_base, V, W, the mean.
#include "ekf_device.h"

#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

__global__ __launch_bounds__(64) void k_loc_associate(const DetIn* __restrict__ det, const int* __restrict__ tagmap,
                                                      const int* __restrict__ nact, int* __restrict__ neff_dev,
                                                      const double* __restrict__ mu, StepIn* __restrict__ step_out,
                                                      AssocOut* __restrict__ assoc_out, LocUnmatched* __restrict__ unmatched,
                                                      unsigned* __restrict__ flags, AssocConfig cfg, int ld, int batch) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x;
  const DetIn& d = det[b];
  const int* tm = tagmap + (long)b * TAGMAX;
  const double* mub = mu + (long)b * ld;
  __shared__ int s_idx[AMAX], s_tag[AMAX], s_cnt[AMAX];
  __shared__ double s_t[AMAX][3], s_err[AMAX];
  __shared__ int c_id[64], c_lm[64], c_ok[64];         // the chunk: tag id, its landmark index in the table (-1: none), 1 = taken / 2 = bad id
  __shared__ double c_t[64][3], c_e[64];
  const int n = nact[b];
  const int nl = (n - 3) / 2;
  int m = 0, un = 0;                                   // (uniform: every lane walks the same sequence)
  unsigned bad = 0;
  unsigned un_seen = 0;                                // lane l < 32: bit i = id 32 l + i was unmatched before in this window
  int un_id = -1;                                      // lane l < AMAX: the l-th distinct unmatched id
  const int count = min(d.count, DMAX);
  if (lane < AMAX) {
    s_idx[lane] = -1;
    s_tag[lane] = -1;
    s_cnt[lane] = 0;
    s_t[lane][0] = s_t[lane][1] = s_t[lane][2] = 0.0;
    s_err[lane] = 0.0;
  }
  for (int q0 = 0; q0 < count; q0 += 64) {
    const int q = q0 + lane;
    int id = -1, lm = -1, ok = 0;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, er = 0.0;
    if (q < count) {
      id = d.tag_id[q];
      t0 = d.pose_t[q][0];
      t1 = d.pose_t[q][1];
      t2 = d.pose_t[q][2];
      er = d.pose_err[q];
      if (id < 0 || id >= TAGMAX) ok = 2;
      else {
        bool ign = false;
        for (int u = 0; u < cfg.n_ignore; ++u) ign |= (cfg.ignore[u] == id);       // :286
        if (!ign && !(t2 * t2 + t0 * t0 > cfg.gate2)) {                            // :289
          ok = 1;
          lm = tm[id];
        }
      }
    }
    WAVE_LDS_SYNC();                                   // (the previous chunk's walk has read its entries)
    c_id[lane] = id;
    c_lm[lane] = lm;
    c_ok[lane] = ok;
    c_t[lane][0] = t0;
    c_t[lane][1] = t1;
    c_t[lane][2] = t2;
    c_e[lane] = er;
    WAVE_LDS_SYNC();
    const int nq = min(64, count - q0);
    for (int u = 0; u < nq; ++u) {                     // in order: what a detection gets depends on the ones before it
      const int ok_u = c_ok[u];
      if (ok_u == 2) { bad |= EKF_FLAG_ASSOC; continue; }
      if (ok_u == 0) continue;
      const int id_u = c_id[u];
      const unsigned long long hit = __ballot(lane < m && s_tag[lane] == id_u);    // the tag's slot in this window, if it has one
      int slot = hit ? __builtin_ctzll(hit) : -1;
      if (slot < 0) {
        const int lm_u = c_lm[u];
        if (lm_u < 0 || lm_u >= nl) {                  // unknown to the table, or a stale row: unmatched (0 <= id_u < TAGMAX here)
          const unsigned bit = 1u << (id_u & 31);
          if (!__ballot(lane == (id_u >> 5) && (un_seen & bit))) {
            if (lane == (id_u >> 5)) un_seen |= bit;
            if (lane == un) un_id = id_u;              // (un >= 64: no lane; only lanes < AMAX are stored)
            ++un;
          }
          continue;
        }
        if (m >= AMAX) { bad |= EKF_FLAG_ASSOC; continue; }
        slot = m++;
        if (lane == 0) {
          s_idx[slot] = lm_u;
          s_tag[slot] = id_u;
        }
      }
      if (lane == 0) {
        s_t[slot][0] += c_t[u][0];                                                  // np.mean(..., axis=0): :315
        s_t[slot][1] += c_t[u][1];
        s_t[slot][2] += c_t[u][2];
        s_err[slot] += c_e[u];                                                      // :317
        s_cnt[slot] += 1;
      }
      WAVE_LDS_SYNC();                                 // (the next detection's search reads the slots)
    }
  }
  if (bad && lane == 0) atomicOr(&flags[b], bad);
  WAVE_LDS_SYNC();
  AssocOut& ao = assoc_out[b];
  const double px = mub[0], py = mub[1], pth = mub[2];         // pose BEFORE the prediction (:331-332)
  if (lane < AMAX) {
    StepIn& so = step_out[(long)(lane / MMAX) * batch + b];
    const int sl = lane % MMAX;
    if (lane < m) {
      const double k = (double)s_cnt[lane];
      const double t0 = s_t[lane][0] / k, t2 = s_t[lane][2] / k;
      const double xr = t2, yr = -t0;                                             // :321
      const double rng = sqrt(xr * xr + yr * yr);                                 // :329
      const double brg = atan2(yr, xr);                                           // :330
      const double xw = px + rng * cos(brg + pth), yw = py + rng * sin(brg + pth);
      const int lm = s_idx[lane];
      so.idx[sl] = lm;
      so.range[sl] = rng;
      so.bearing[sl] = brg;
      ao.idx[lane] = lm;
      ao.tag_id[lane] = s_tag[lane];
      ao.xw[lane] = xw;
      ao.yw[lane] = yw;
      ao.err[lane] = s_err[lane] / k;
      ao.range[lane] = rng;
      ao.bearing[lane] = brg;
    } else {
      so.idx[sl] = 0;
      so.range[sl] = 0.0;
      so.bearing[sl] = 0.0;
    }
    unmatched[b].tag_id[lane] = lane < un ? un_id : -1;
  }
  if (lane == 0) {
    int bound = neff_dev[b];
    for (int u = 0; u < m; ++u) bound = max(bound, 3 + 2 * (s_idx[u] + 1));
    bound = min(bound, n);
    neff_dev[b] = bound;
    StepIn& s0 = step_out[b];
    StepIn& s1 = step_out[(long)batch + b];
    s0.lin = d.lin;
    s0.ang = d.ang;
    s0.m = min(m, MMAX);
    s0.flags = FLAG_PREDICT | FLAG_UPDATE;
    s0.neff = cfg.active_bound ? bound : n;
    s0.pad = 0;
    s1.lin = 0.0;                                      // the landmarks beyond the first pass: an update without a prediction
    s1.ang = 0.0;
    s1.m = max(m - MMAX, 0);
    s1.flags = FLAG_UPDATE;
    s1.neff = s0.neff;
    s1.pad = 0;
    ao.m = m;
    ao.n_after = n;
    unmatched[b].total = un;
    unmatched[b].pad = 0;
  }
}

void launch_loc_associate(hipStream_t st, const BankView& k, const DetIn* det, const int* tagmap, int* neff_dev, const double* mu,
                          StepIn* step_out, AssocOut* assoc_out, LocUnmatched* unmatched, const AssocConfig& cfg) {
  hipLaunchKernelGGL(k_loc_associate, dim3(k.batch), dim3(64), 0, st, det, tagmap, k.nact, neff_dev, mu, step_out, assoc_out,
                     unmatched, k.flags, cfg, k.ld, k.batch);
}

}  // namespace ekf
