// The device-side front ends that turn one window of raw AprilTag detections into the StepIn records a solve consumes (gfx950,
// wave64): k_associate for ekf_step_detections, on a map that grows, k_loc_associate for ekf_localize_detections, on a FROZEN
// one, and k_hyp_associate for a hypothesis bank's windows (ekf_hypotheses_step_detections, ekf_hypotheses_detections_upload), on
// the bank's frozen map and for every hypothesis at once.  One workgroup of ONE wave per window: grid = batch for the first two,
// grid = windows for the third.  All run the walk of ekf_det_walk.h -- the DetIn records in chunks of 64, the ignore list, the
// gate, ids outside [0, TAGMAX), one slot per distinct tag in order of first appearance, the sums, the per-tag mean, range,
// bearing and world guess, the two StepIn records and the AssocOut record -- so a tag's averaged (range, bearing) has the same
// bits on all of them.  What is written here is what differs: what a detection gets whose tag has no slot in the window yet,
// and what the window does to the filter.
#include "ekf_device.h"

#include "ekf_det_walk.h"
#include "ekf_devfn.h"
#include "ekf_launch.h"

namespace ekf {

// ---------------------------------------------------------------------------------------------
// k_associate: association, gate, averaging and augmentation of one window (src/replay_no_ros.py:280-360).  The reference's
// dictionaries have no limits (:280-301) and its normal mode hands over a 0.7 s window of every camera frame (:17: 21 frames x
// every tag in view), so up to EKF_DMAX = 256 detections are walked and up to EKF_AMAX = 32 distinct tags are taken (two update
// passes of EKF_MMAX landmarks).  A tag the table does not know gets the next landmark index (:294-295) and an entry in the
// table, unless the state is full; the new landmarks' means, the zeroing of their rows / columns and the new diagonal (:341-360)
// are spread over the lanes.  Writes the StepIn records, the tags_positions record, the new state size and the active bound.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_associate(const DetIn* __restrict__ det, int* __restrict__ tagmap,
                                                  int* __restrict__ nact, int* __restrict__ neff_dev,
                                                  double* __restrict__ mu, double* __restrict__ P,
                                                  double* __restrict__ V, double* __restrict__ W,
                                                  StepIn* __restrict__ step_out,
                                                  AssocOut* __restrict__ assoc_out,
                                                  unsigned* __restrict__ flags, AssocConfig cfg, int ld,
                                                  long pstride, int n_max, int pending_k, int batch) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const DetIn& d = det[b];
  int* tm = tagmap + (long)b * TAGMAX;
  double* mub = mu + (long)b * ld;
  double* Pb = P + (long)b * pstride;
  double* Vb = V + (long)b * KTOT * ld;
  double* Wb = W + (long)b * KTOT * ld;
  __shared__ DetWalkShared sh;
  const int n_old = nact[b];
  const int nl_old = (n_old - 3) / 2;
  int nl = nl_old;                                     // (uniform)
  const int m = det_walk(sh, d, tm, cfg, min(d.count, DMAX), flags + b, lane, [&](int id, int lm, int m, unsigned& bad) {
    // a detection that cannot be taken is dropped BEFORE it gets a landmark index: an index handed out here with no
    // measurement behind it would leave an uninitialised landmark in the state
    if (m >= AMAX) { bad |= EKF_FLAG_ASSOC; return -1; }
    if (lm < 0) {                                      // (a tag new in this window has a slot from its first detection on and never comes here again)
      if (3 + 2 * (nl + 1) > n_max) { bad |= EKF_FLAG_ASSOC; return -1; }          // :294-295
      lm = nl++;
      if (lane == 0) tm[id] = lm;
    }
    return lm;
  });
  const int n_new = 3 + 2 * nl;
  AssocOut& ao = assoc_out[b];
  const double px = mub[0], py = mub[1], pth = mub[2];         // pose BEFORE the prediction (:331-332)
  if (lane < AMAX) {
    const DetTag t = det_tag_out(sh, lane, m, px, py, pth, step_out, batch, b, ao);
    if (t.lm >= nl_old) {                                                         // :359-360
      mub[3 + 2 * t.lm] = t.xw;
      mub[4 + 2 * t.lm] = t.yw;
    }
  }
  // augmentation (:341-360): zero the new rows/columns, set the new diagonal; pending ranks see zeros
  const int dn = n_new - n_old;
  const int ld16 = ld >> 4;
  for (long e = lane; e < (long)n_new * dn; e += 64) {
    const int r = (int)(e / dn), q = n_old + (int)(e - (long)r * dn);
    Pb[p_index(ld, r, q)] = (r == q) ? cfg.init_var : 0.0;
    if (r < n_old) Pb[p_index(ld, q, r)] = 0.0;
  }
  for (int e = lane; e < pending_k * dn; e += 64) {
    const int k = e / dn, q = n_old + (e - k * dn);
    Vb[(long)k * ld + q] = 0.0;
    Wb[wm_index(ld16, k, q)] = 0.0;
  }
  if (lane == 0) {
    det_tail(sh, d, cfg, m, n_new, neff_dev, step_out, batch, b, ao);
    nact[b] = n_new;
  }
}

void launch_associate(hipStream_t st, const BankView& k, const DetIn* det, int* tagmap, int* neff_dev, double* mu, StepIn* step_out,
                      AssocOut* assoc_out, const AssocConfig& cfg, int n_max, int pending_k) {
  hipLaunchKernelGGL(k_associate, dim3(k.batch), dim3(64), 0, st, det, tagmap, k.nact, neff_dev, mu, k.P, k.V, k.W, step_out,
                     assoc_out, k.flags, cfg, k.ld, k.pstride, n_max, pending_k, k.batch);
}

// The admit rule of a FROZEN map's walk (k_loc_associate, k_hyp_associate) and what it keeps of the tags the map does not hold.
// A tag the table does not know, or whose entry points at or beyond the nl landmarks of the map (a stale row), is UNMATCHED -- no
// slot, no flag; its id is kept, distinct ids in order of first appearance.  More than AMAX distinct MATCHED tags: the surplus
// is dropped with EKF_FLAG_ASSOC, as in mapping.  Which ids were already seen as unmatched is a 1024-bit set held in registers
// (lane l < 32 holds ids 32 l .. 32 l + 31), the list itself one id per lane: the only LDS traffic is the walk's.
struct LocUnseen {
  int total = 0;                                       // (uniform) the distinct unmatched ids so far
  unsigned seen = 0;                                   // lane l < 32: bit i = id 32 l + i was unmatched before in this window
  int mine = -1;                                       // lane l: the l-th distinct unmatched id (only lanes < AMAX are stored)
  __device__ __forceinline__ int admit(int lane, int nl, int id, int lm, int m, unsigned& bad) {
    if (lm < 0 || lm >= nl) {                          // unknown to the table, or a stale row: unmatched (0 <= id < TAGMAX here)
      const unsigned bit = 1u << (id & 31);
      if (!__ballot(lane == (id >> 5) && (seen & bit))) {
        if (lane == (id >> 5)) seen |= bit;
        if (lane == total) mine = id;                  // (total >= 64: no lane)
        ++total;
      }
      return -1;
    }
    if (m >= AMAX) { bad |= EKF_FLAG_ASSOC; return -1; }
    return lm;
  }
  __device__ __forceinline__ void store_id(int lane, LocUnmatched& u) const { u.tag_id[lane] = lane < total ? mine : -1; }   // lane < AMAX
  __device__ __forceinline__ void store_total(LocUnmatched& u) const {                                                       // lane 0
    u.total = total;
    u.pad = 0;
  }
};

// ---------------------------------------------------------------------------------------------
// k_loc_associate: :280-337 against a frozen map, and nothing of :341-360 -- no landmark is ever added.  A tag the table does
// not know, or whose entry points at or beyond the trajectory's landmark count (a stale row), is UNMATCHED -- no slot, no flag,
// nothing changes; its id goes to the trajectory's LocUnmatched record, distinct ids in order of first appearance (the first
// AMAX of them; `total` counts all).  More than AMAX distinct MATCHED tags: the surplus is dropped with EKF_FLAG_ASSOC, as in
// mapping (LocUnseen).
// Written: step_out[b] (FLAG_PREDICT | FLAG_UPDATE, up to MMAX observations) and step_out[batch + b] (the update-only rest),
// assoc_out[b] (the matched tags, n_after = n), unmatched[b], neff_dev[b] (raised over the matched landmarks, capped at n: a
// consider update correlates the pose with every landmark it names, and only the device knows which those are), the sticky flag.
// NOT written: tagmap, nact, P_base, V, W, the mean.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_loc_associate(const DetIn* __restrict__ det, const int* __restrict__ tagmap,
                                                      const int* __restrict__ nact, int* __restrict__ neff_dev,
                                                      const double* __restrict__ mu, StepIn* __restrict__ step_out,
                                                      AssocOut* __restrict__ assoc_out, LocUnmatched* __restrict__ unmatched,
                                                      unsigned* __restrict__ flags, AssocConfig cfg, int ld, int batch) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const DetIn& d = det[b];
  const double* mub = mu + (long)b * ld;
  __shared__ DetWalkShared sh;
  const int n = nact[b];
  const int nl = (n - 3) / 2;
  LocUnseen un;
  const int m = det_walk(sh, d, tagmap + (long)b * TAGMAX, cfg, min(d.count, DMAX), flags + b, lane,
                         [&](int id, int lm, int m, unsigned& bad) { return un.admit(lane, nl, id, lm, m, bad); });
  AssocOut& ao = assoc_out[b];
  const double px = mub[0], py = mub[1], pth = mub[2];         // pose BEFORE the prediction (:331-332)
  if (lane < AMAX) {
    det_tag_out(sh, lane, m, px, py, pth, step_out, batch, b, ao);
    un.store_id(lane, unmatched[b]);
  }
  if (lane == 0) {
    det_tail(sh, d, cfg, m, n, neff_dev, step_out, batch, b, ao);
    un.store_total(unmatched[b]);
  }
}

void launch_loc_associate(hipStream_t st, const BankView& k, const DetIn* det, const int* tagmap, int* neff_dev, const double* mu,
                          StepIn* step_out, AssocOut* assoc_out, LocUnmatched* unmatched, const AssocConfig& cfg) {
  hipLaunchKernelGGL(k_loc_associate, dim3(k.batch), dim3(64), 0, st, det, tagmap, k.nact, neff_dev, mu, step_out, assoc_out,
                     unmatched, k.flags, cfg, k.ld, k.batch);
}

// ---------------------------------------------------------------------------------------------
// k_hyp_associate: k_loc_associate's walk for a hypothesis bank.  The bank's tag-table row and map are frozen and the walk reads
// no pose, so ONE walk of a window serves every hypothesis: window w (blockIdx.x; `windows` = the grid: 1 for
// ekf_hypotheses_step_detections, the steps of an ekf_hypotheses_detections_upload) against the bank's row `tagrow` with
// LocUnseen's admit rule on the map's (n - 3) / 2 landmarks.
// Written: step_out[w] (FLAG_PREDICT | FLAG_UPDATE, lin / ang of the window, up to MMAX observations) and step_out[windows + w]
// (the update-only rest) -- the shared records k_hyp_solve reads with rec_stride 0; StepIn::neff = n, which k_hyp_solve does not
// read: a hypothesis's bound lives in its HypState and the solve raises it over the record's landmarks --, assoc_out[w] (the
// matched tags in update order, n_after = n), unmatched[w] and flags[w] (written whole: 0, or EKF_FLAG_ASSOC for an id outside
// [0, TAGMAX) or a surplus tag).  The bank has no single pose: AssocOut::xw / yw are formed with the pose (0, 0, 0), i.e. they
// are the tag's averaged position in the ROBOT frame (range cos bearing, range sin bearing).
// NOT written: the bank's map, its tag row, any HypState, X.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hyp_associate(const DetIn* __restrict__ det, const int* __restrict__ tagrow,
                                                      StepIn* __restrict__ step_out, AssocOut* __restrict__ assoc_out,
                                                      LocUnmatched* __restrict__ unmatched, unsigned* __restrict__ flags,
                                                      AssocConfig cfg, int n, int windows) {
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= windows) return;                            // (the whole wave)
  const DetIn& d = det[w];
  __shared__ DetWalkShared sh;
  const int nl = (n - 3) / 2;
  if (lane == 0) flags[w] = 0u;                        // (lane 0 too raises it, behind this store: det_walk's atomicOr)
  LocUnseen un;
  const int m = det_walk(sh, d, tagrow, cfg, max(0, min(d.count, DMAX)), flags + w, lane,
                         [&](int id, int lm, int m, unsigned& bad) { return un.admit(lane, nl, id, lm, m, bad); });
  AssocOut& ao = assoc_out[w];
  if (lane < AMAX) {
    det_tag_out(sh, lane, m, 0.0, 0.0, 0.0, step_out, windows, w, ao);
    un.store_id(lane, unmatched[w]);
  }
  if (lane == 0) {
    det_heads(d, m, n, n, step_out, windows, w, ao);
    un.store_total(unmatched[w]);
  }
}

void launch_hyp_associate(hipStream_t st, const HypView& v, const int* tagrow, const DetIn* det, int windows, StepIn* step_out,
                          AssocOut* assoc_out, LocUnmatched* unmatched, unsigned* flags, const AssocConfig& cfg) {
  hipLaunchKernelGGL(k_hyp_associate, dim3(windows), dim3(64), 0, st, det, tagrow, step_out, assoc_out, unmatched, flags, cfg, v.n,
                     windows);
}

}  // namespace ekf
