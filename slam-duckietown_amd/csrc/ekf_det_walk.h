// The walk over one window of raw AprilTag detections (src/replay_no_ros.py:280-337), shared by the three kernels that run it
// (ekf_loc_assoc.hip): k_associate on a growing map (ekf_step_detections), k_loc_associate on a frozen one
// (ekf_localize_detections) and k_hyp_associate on a hypothesis bank's (ekf_hypotheses_step_detections / _detections_upload).
// ONE wave per window; every lane calls every function here.
//   det_walk      the detections in chunks of 64 -- per chunk every lane fetches ITS detection (id, the id's landmark index from
//                 the tag table, IGNORE_TAGS, the gate): one memory round trip for 64 detections -- then, detection by detection
//                 and without touching memory, what depends on their ORDER: one slot per distinct tag in order of first
//                 appearance (:294-295; the update order, :436), found by all lanes at once, and the slot's sums.  What a
//                 detection gets whose tag has no slot in this window yet is the caller's `admit`.
//   det_tag_out   lane = slot: the sums divided by the count, xr = t2, yr = -t0, sqrt, atan2, the world guess from the pose
//                 BEFORE the prediction, into the slot's places of the two StepIn records and of the AssocOut record.
//   det_tail      (lane 0) the active bound raised over the window's landmarks and the heads of the two StepIn records
//                 (det_heads: the heads alone, where the bound lives elsewhere).
// The kernels give a tag the same averaged (range, bearing) bits because this is the only statement of that arithmetic; it
// runs without contraction, and `#pragma clang fp contract(off)` is lexical: every function with arithmetic carries its own.
#pragma once
#include "ekf_device.h"

#include "ekf_devfn.h"

namespace ekf {

struct DetWalkShared {                                 // (every array 16-byte aligned, as LDS arrays of their own are: the walk's 128-bit reads)
  alignas(16) int idx[AMAX], tag[AMAX], cnt[AMAX];     // per slot: landmark index, tag id, detections summed
  alignas(16) double t[AMAX][3], err[AMAX];            // per slot: the sums of pose_t and pose_err
  alignas(16) int c_id[64], c_lm[64], c_ok[64];        // the chunk: tag id, its landmark index in the table (-1: none), 1 = taken / 2 = bad id
  alignas(16) double c_t[64][3], c_e[64];
};

// Walks the first `count` detections of `d` against the tag table `tm` as it stood before this window; returns the number of
// slots taken (uniform: every lane walks the same sequence).  `admit(id, lm, m, bad)`, called by every lane alike for a taken
// detection whose tag has no slot yet (lm: the table's entry, m: the slots so far): the landmark index of the new slot, or a
// negative value when the detection gets none -- the order of its checks is the kernel's behaviour, and it raises `bad` itself.
// Ids outside [0, TAGMAX) raise EKF_FLAG_ASSOC; what was raised goes to *flag.
template <class Admit>
__device__ __forceinline__ int det_walk(DetWalkShared& sh, const DetIn& d, const int* tm, const AssocConfig& cfg, int count,
                                        unsigned* flag, int lane, Admit admit) {
#pragma clang fp contract(off)
  int m = 0;
  unsigned bad = 0;
  if (lane < AMAX) {
    sh.idx[lane] = -1;
    sh.tag[lane] = -1;
    sh.cnt[lane] = 0;
    sh.t[lane][0] = sh.t[lane][1] = sh.t[lane][2] = 0.0;
    sh.err[lane] = 0.0;
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
    sh.c_id[lane] = id;
    sh.c_lm[lane] = lm;
    sh.c_ok[lane] = ok;
    sh.c_t[lane][0] = t0;
    sh.c_t[lane][1] = t1;
    sh.c_t[lane][2] = t2;
    sh.c_e[lane] = er;
    WAVE_LDS_SYNC();
    const int nq = min(64, count - q0);
    for (int u = 0; u < nq; ++u) {                     // in order: what a detection gets depends on the ones before it
      const int ok_u = sh.c_ok[u];
      if (ok_u == 2) { bad |= EKF_FLAG_ASSOC; continue; }
      if (ok_u == 0) continue;
      const int id_u = sh.c_id[u];
      const unsigned long long hit = __ballot(lane < m && sh.tag[lane] == id_u);   // the tag's slot in this window, if it has one
      int slot = hit ? __builtin_ctzll(hit) : -1;
      if (slot < 0) {
        const int lm_u = admit(id_u, sh.c_lm[u], m, bad);
        if (lm_u < 0) continue;
        slot = m++;
        if (lane == 0) {
          sh.idx[slot] = lm_u;
          sh.tag[slot] = id_u;
        }
      }
      if (lane == 0) {
        // (the detection is read whole before the first sum is written: the arrays are members of one object, and a store to
        //  one keeps the loads of another behind it -- two more LDS round trips per detection on the walk's serial path: 1.5 us of k_loc_associate's 16)
        const double c0 = sh.c_t[u][0], c1 = sh.c_t[u][1], c2 = sh.c_t[u][2], ce = sh.c_e[u];
        const double s0 = sh.t[slot][0], s1 = sh.t[slot][1], s2 = sh.t[slot][2], se = sh.err[slot];
        const int sc = sh.cnt[slot];
        sh.t[slot][0] = s0 + c0;                                                    // np.mean(..., axis=0): :315
        sh.t[slot][1] = s1 + c1;
        sh.t[slot][2] = s2 + c2;
        sh.err[slot] = se + ce;                                                     // :317
        sh.cnt[slot] = sc + 1;
      }
      WAVE_LDS_SYNC();                                 // (the next detection's search reads the slots)
    }
  }
  if (bad && lane == 0) atomicOr(flag, bad);
  WAVE_LDS_SYNC();
  return m;
}

// Slot `lane` of the window (lane < AMAX): its averaged observation into place lane % MMAX of record lane / MMAX of `step_out`
// (zeros beyond the m slots taken) and into `ao`.  (px, py, pth): the pose BEFORE the prediction (:331-332).  Returns the slot's
// landmark and its world guess, lm = -1 beyond m.
struct DetTag {
  int lm;
  double xw, yw;
};
__device__ __forceinline__ DetTag det_tag_out(const DetWalkShared& sh, int lane, int m, double px, double py, double pth,
                                              StepIn* step_out, int batch, int b, AssocOut& ao) {
#pragma clang fp contract(off)
  DetTag r{-1, 0.0, 0.0};
  StepIn& so = step_out[(long)(lane / MMAX) * batch + b];
  const int sl = lane % MMAX;
  if (lane < m) {
    const double k = (double)sh.cnt[lane];
    const double t0 = sh.t[lane][0] / k, t2 = sh.t[lane][2] / k;
    const double xr = t2, yr = -t0;                                               // :321
    const double rng = sqrt(xr * xr + yr * yr);                                   // :329
    const double brg = atan2(yr, xr);                                             // :330
    r.xw = px + rng * cos(brg + pth);
    r.yw = py + rng * sin(brg + pth);
    r.lm = sh.idx[lane];
    so.idx[sl] = r.lm;
    so.range[sl] = rng;
    so.bearing[sl] = brg;
    ao.idx[lane] = r.lm;
    ao.tag_id[lane] = sh.tag[lane];
    ao.xw[lane] = r.xw;
    ao.yw[lane] = r.yw;
    ao.err[lane] = sh.err[lane] / k;
    ao.range[lane] = rng;
    ao.bearing[lane] = brg;
  } else {
    so.idx[sl] = 0;
    so.range[sl] = 0.0;
    so.bearing[sl] = 0.0;
  }
  return r;
}

// (lane 0) the heads of a window's two StepIn records -- [b]: the prediction and the first MMAX landmarks, [batch + b]: the
// rest, an update without a prediction -- with the active bound `neff` both carry, and of `ao`.
__device__ __forceinline__ void det_heads(const DetIn& d, int m, int neff, int n_after, StepIn* step_out, int batch, int b,
                                          AssocOut& ao) {
  StepIn& s0 = step_out[b];
  StepIn& s1 = step_out[(long)batch + b];
  s0.lin = d.lin;
  s0.ang = d.ang;
  s0.m = min(m, MMAX);
  s0.flags = FLAG_PREDICT | FLAG_UPDATE;
  s0.neff = neff;
  s0.pad = 0;
  s1.lin = 0.0;
  s1.ang = 0.0;
  s1.m = max(m - MMAX, 0);
  s1.flags = FLAG_UPDATE;
  s1.neff = neff;
  s1.pad = 0;
  ao.m = m;
  ao.n_after = n_after;
}

// (lane 0) the trajectory's active bound raised over the window's landmarks and capped at the state's size after the window,
// then det_heads with it.
__device__ __forceinline__ void det_tail(const DetWalkShared& sh, const DetIn& d, const AssocConfig& cfg, int m, int n_after,
                                         int* neff_dev, StepIn* step_out, int batch, int b, AssocOut& ao) {
  int bound = neff_dev[b];
  for (int u = 0; u < m; ++u) bound = max(bound, 3 + 2 * (sh.idx[u] + 1));
  bound = min(bound, n_after);
  neff_dev[b] = bound;
  det_heads(d, m, cfg.active_bound ? bound : n_after, n_after, step_out, batch, b, ao);
}

}  // namespace ekf
