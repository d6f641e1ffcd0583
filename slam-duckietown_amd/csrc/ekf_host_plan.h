// Host-side planning logic of the EKF-SLAM core: everything that decides WHAT is launched -- the covariance pass's kernel and
// launch shape, its work queues and static shares, the form of a step's update, how many steps of an uploaded stream form a
// fused cadence and what follows each one, the small-state kernel, the step records and their active bound, the validation of
// observation lists -- as plain C++ on plain data (no HIP type, no device call).  ekf_api.hip's handle derives from HostPlan
// and calls these, the launchers only map their answers to kernel instantiations; the same header compiles with plain g++
// (-DEKF_HOST_ONLY), and tests/host_plan_check.cpp runs it under -fsanitize=address,undefined: enumerations of the queue /
// share arithmetic plus randomised invariants of the planning functions (tests/test_cpu_host.py builds and runs it).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "ekf_device.h"

namespace ekf {

constexpr int RS_ROWS = 128;            // rows of a slab of the row-slab pass = 8 waves x 16

// The state of the fused cadences of ekf_stream_run, carried from cadence to cadence and from run to run: what
// plan_cadence_launches reads and advances (plain counters and parities: the buffers they select are the handle's).
struct CadRun {
  int cpar = 0;                   // which copy of the records (dcad2) and pose rows (dprow3) the next cadence uses: flips per cadence
  unsigned sigma = 0;             // chained transitions so far (the value the run's counters SYNC_SOLVE / SYNC_PASS carry)
  unsigned gather_count = 0;      // gather workgroups launched so far (what the next chain workgroups wait for)
  // a cadence's inputs formed one cadence ahead (CadPre): two copies, by the cadence's serial number (pre_serial: whose inputs a
  // copy holds; serials count every cadence of the handle)
  long cad_serial = 0;
  long pre_serial[2] = {-1, -1};
  bool aux_pass = false;          // a covariance pass is in flight on the second stream (JOIN_AUX / join_aux makes the handle's wait)
  // statistics
  long cadences = 0, cadence_traj_steps = 0;   // fused cadences launched, trajectory-steps they completed
  long lookaheads = 0;            // cadences whose solve ran beside the previous pass (look-ahead and chained)
  long chained = 0;               // ... of those: cadences whose block came from k_chain_cad
  long w_from_v_passes = 0;       // passes that formed W from V ("w_from_v")
};

// What the planning functions read of a handle (ekf_handle derives from this).
struct HostPlan {
  int device = 0, n_max = 0, ld = 0, rows = 0, batch = 0;
  long pstride = 0;
  ekf_config cfg{};
  int cu_count = 0;
  int pending_k = 0, pending_steps = 0;   // ranks / steps appended to (V, W) since the last flush
  std::vector<int> n;             // state size per trajectory
  std::vector<int> neff_enq;      // active bound of the last ENQUEUED step (what dso[b].neff holds)
  std::vector<int> neff;          // active bound per trajectory (<= n): indices beyond were never correlated
  std::vector<int> floor_host;    // what dfloor holds (see push_floor)
  bool sizes_dirty = false;       // the device grew the state: n / neff must be read back before use
  int stream_steps = 0;
  std::vector<int> stream_mhi;    // per step: most observations of any trajectory
  std::vector<unsigned char> stream_m;   // per (step, trajectory): observations the kernels will process (0 with the measurement model off)
  std::vector<int> stream_own;    // per (step, trajectory): active bound from the stream's OWN observations up to that step
  std::vector<int> stream_maxlm;  // per trajectory: landmarks the stream needs in the state (largest index + 1)
  int opt_active_bound = 1;       // 0 = always treat the whole state as active
  int opt_rank_limit = KTOT;      // automatic cadence: flush when the next step would exceed this many ranks
  int opt_pass_kernel = -1;       // -1 = auto, 0 = k_flush (column strips), 2 = k_flush_rs (row slabs)
  int opt_fused_step = 1;         // 1 = one launch per step where the launch is small (k_step_split), 0 = always two
  int opt_fused_cadence = 1;      // 1 = uploaded streams run whole cadences as one solve + one panel launch (ekf_cadence.hip)
  int opt_lookahead = 1;
  int opt_chain = 1;              // 1 = chained solves where a pass can leave CUs to a solve beside it (plan_chain_run)
  // 1 = where a fused cadence's covariance pass follows its panel launch at once, in the row-slab form, the panel launch writes V
  // only and the pass forms its W fragments from V and the records' S^-1 (half of the panel launch's stores); bit-identical
  int opt_w_from_v = 1;
  int opt_panel_shape = 0;        // diagnostics: 0 = the panel launch's shape by its size; 1 k_panels_cad_ks, 2 k_panels_cad<1>, 3 k_panels_cad<4> whatever the size
  int opt_panel_tform = 1;        // 1 = a chained cadence's panel launch in the latency regime takes the triangular-solve form (k_panels_cad_tf)
  int opt_col_gather = 1;         // 1 = the solve gathers the panel launch's mirrored column entries beside it, 0 = the panel launch gathers everything itself
  // the piece of a run in flight, decided before its first cadence (ekf_api.hip: prepare_piece): its solves record the transforms
  // (every solve is k_solve_cad<true>), and the gather workgroups per trajectory of its chain launches (chain_gather_workgroups)
  bool chain_run = false;
  int chain_gw = 1;
  CadRun run;                     // the fused cadences' state (plan_cadence_launches)
  int opt_small_state = 1;        // 1 = small filters (n_max <= 79: up to 38 landmarks) run in ONE workgroup, P in LDS (ekf_small.hip)
  int opt_rows_per_block = 0;     // 0 = auto (flush kernel: rows per workgroup, multiple of 16)
  int opt_pass_chunk = 0;         // 0 = auto (k_flush_rs: strips per unit)
  int opt_pass_workgroups = 0;    // 0 = one per CU (k_flush_rs: persistent workgroups; fewer leaves CUs to other streams)
  int opt_flush_every = 0;        // 0 = auto; k = flush the pending low-rank update after k steps
  int opt_streaming = -1;         // -1 = auto (by working-set size), 0 = resident kernel, 1 = nontemporal kernel
};

// ---- the work queues of k_flush_rs (one per XCD): how many units queue g2 holds and which unit its u-th one is ----
// By `mode`:
//   0  uniform ("pass_chunk" set, or fewer than 8 trajectories): trajectories g2, g2 + 8, ..., every slab in `nch`
//      chunks, chunk-major;
//   1  pairs (batch a multiple of 8): trajectories g2, g2 + 8, ... one after the other, whole slabs longest
//      first -- the workgroup that got the longest slab of one trajectory gets the shortest of the next; the last of
//      an odd number (8 trajectories: the only one) has no partner and its slabs, only they, are cut into `nch` chunks;
//   2  dealt (any other batch): the queue's own trajectories among the first 8 * (batch / 8), plus the slabs
//      rb = (g2 - j) mod 8, + 8, ... of each of the batch-modulo-8 last trajectories j -- every queue carries the same
//      work -- whole slabs, longest first over ALL of them (slab index major): list scheduling in that order is
//      as good as the longest slab allows; the price is that an XCD walks the V strips of several trajectories at
//      once (1-3 % on the batches where mode 1 applies, hence not used there).  N=2000, 20 trajectories: 496 us
//      against 524 us with mode 1, 28: 662 against 700; 24 (mode 1): 560 against 584 with mode 2.
//   3  dealt halves (8 < batch <= 12, where one trajectory per queue leaves a workgroup less than two slabs): as mode 2,
//      but every slab in two chunks of cs = 2 h strips; chunk 1 of slab rb is as long as slab rb + h, so handing out
//      "chunk 0 of slab v, chunk 1 of slab v - h" for v = 0, 1, ... is again longest first.  (`nch` carries h.)
// A unit is (trajectory * nrb + slab) * 1024 + chunk, chunk = 1023 for a whole slab.  Plain integer functions, also
// compiled for the host: tests/test_cpu_host.py enumerates them through ekf_debug_pass_units and checks that every
// (trajectory, slab, chunk) comes exactly once.
__host__ __device__ inline int rs_queue_count(int g2, int batch, int nrb, int nch, int mode) {
  const int upt = nrb * nch;
  if (mode == 3) return 2 * rs_queue_count(g2, batch, nrb, 1, 2);
  if (mode == 2) {
    const int nfull = batch >> 3, nleft = batch & 7;
    int dealt = 0;                                     // slabs rb < nrb with ((g2 - rb) & 7) < nleft
    for (int j = 0; j < nleft; ++j) {
      const int r0 = (g2 - j) & 7;
      dealt += (r0 < nrb) ? ((nrb - r0 + 7) >> 3) : 0;
    }
    return nfull * nrb + dealt;
  }
  const int tq = (g2 < batch) ? ((batch - g2 + 7) >> 3) : 0;
  if (mode == 0) return tq * upt;
  const int lone = tq & 1;
  return (tq - lone) * nrb + lone * upt;
}
__host__ __device__ inline int rs_queue_unit(int g2, int u, int batch, int nrb, int nch, int mode) {
  const int upt = nrb * nch;
  int r = u;
  if (mode == 3) {
    const int nfull = batch >> 3, nleft = batch & 7, h = nch;
    for (int v = 0; v < nrb + h; ++v) {                // (a few dozen iterations, once per unit, one thread)
      for (int chunk = 0; chunk < 2; ++chunk) {
        const int rb = v - chunk * h;
        if (rb < 0 || rb >= nrb) continue;
        const int j = (g2 - rb) & 7;
        const int ci = nfull + (j < nleft ? 1 : 0);
        if (r < ci) return ((r < nfull ? g2 + 8 * r : 8 * nfull + j) * nrb + rb) * 1024 + chunk;
        r -= ci;
      }
    }
    return -1;                                         // (not reached for u < rs_queue_count)
  }
  if (mode == 0) {
    const int t = r / upt;
    r -= t * upt;
    return ((g2 + 8 * t) * nrb + r % nrb) * 1024 + (nch > 1 ? r / nrb : 1023);
  }
  if (mode == 2) {
    // slab-index major: a block of 8 consecutive slabs holds 8 * nfull own units and nleft dealt ones
    const int nfull = batch >> 3, nleft = batch & 7;
    const int per = 8 * nfull + nleft, blk = r / per;
    r -= blk * per;
    for (int i = 0; i < 8; ++i) {
      const int rb = 8 * blk + i, j = (g2 - rb) & 7;
      const int ci = nfull + (j < nleft ? 1 : 0);
      if (r < ci) return ((r < nfull ? g2 + 8 * r : 8 * nfull + j) * nrb + rb) * 1024 + 1023;
      r -= ci;
    }
    return -1;                                         // (not reached for u < rs_queue_count)
  }
  const int tq = (g2 < batch) ? ((batch - g2 + 7) >> 3) : 0;
  const int whole = (tq - (tq & 1)) * nrb;
  if (r < whole) return ((g2 + 8 * (r / nrb)) * nrb + r % nrb) * 1024 + 1023;
  r -= whole;
  return ((g2 + 8 * (tq - 1)) * nrb + r % nrb) * 1024 + r / nrb;
}
// ---- mode 4: equal static shares (a few LONG trajectories, e.g. N = 8000 x 1: 126 slabs for 256 CUs) ----
// Whole slabs cannot balance 256 workgroups there, and dynamically handed-out chunks end in a tail as long as a chunk
// while every unit boundary costs about two strips' worth (pipeline fill and drain).  So the batch's strips -- trajectory
// by trajectory, slab by slab, each slab from its right end to the diagonal -- are cut into one contiguous share per
// workgroup of equal COST (strips + RS_PIECE_COST per piece): a share is a handful of pieces (trajectory, slab, first
// strip, strips), at most RS_PIECES.  No queue, no atomics; the table depends on (batch, n_hi, workgroups) only and is
// cached on the device.  Returns the pieces of the longest share, 0 if some share would need more than RS_PIECES.
// (Groups of 2 / 4 / 8 workgroups walking ADJACENT strips of the same rows in step -- longer contiguous row segments in
//  flight at any time -- were measured at N = 8000 x 1: 401 / 439 / 471 us against 391 us: not adopted.)
constexpr int RS_PIECES = 16;
constexpr int RS_PIECE_COST = 2;
inline int build_pass_shares(int batch, int n_hi, int workgroups, int* out /* workgroups x RS_PIECES x 4 */) {
  const int nrb = (n_hi + RS_ROWS - 1) / RS_ROWS, s_last = (n_hi - 1) >> 6;
  long rem_strips = 0;
  for (int rb = 0; rb < nrb; ++rb) rem_strips += s_last - 2 * rb + 1;
  rem_strips *= batch;
  long rem_slabs = (long)batch * nrb;                  // slabs not yet started
  for (int i = 0; i < workgroups * RS_PIECES * 4; ++i) out[i] = 0;
  int w = 0, k = 0, longest = 0;
  // what a share may cost: what is left (strips + a piece per slab still to start + a piece per share still to open,
  // the continuation of a slab cut by a share boundary) over the shares left -- recomputed whenever a share is opened
  auto budget_now = [&](int slab_left) {
    const long left = rem_strips + RS_PIECE_COST * (rem_slabs + (slab_left > 0 ? 1 : 0) + (workgroups - w - 1));
    return (double)left / (double)(workgroups - w);
  };
  double budget = budget_now(0), used = 0.0;
  for (int b = 0; b < batch; ++b)
    for (int v = 0; v < nrb; ++v) {
      // slabs of a trajectory alternately from both ends (longest, shortest, second longest, ...): the many short slabs
      // near the diagonal's end do not pile up in one share
      const int rb = (v & 1) ? nrb - 1 - (v >> 1) : (v >> 1);
      int S = s_last - 2 * rb + 1, start = 0;
      --rem_slabs;
      while (S > 0) {
        if (k > 0 && used + RS_PIECE_COST + 1 > budget && w + 1 < workgroups) {   // no room for even one strip: next share
          ++w;
          k = 0;
          used = 0.0;
          budget = budget_now(S);
        }
        const int room = w + 1 < workgroups ? (int)(budget - used - RS_PIECE_COST + 0.5) : S;
        const int cnt = room < 1 ? 1 : (room < S ? room : S);
        if (k >= RS_PIECES) return 0;
        int* pc = out + ((long)w * RS_PIECES + k) * 4;
        pc[0] = b;
        pc[1] = rb;
        pc[2] = start;
        pc[3] = cnt;
        ++k;
        longest = k > longest ? k : longest;
        used += cnt + RS_PIECE_COST;
        start += cnt;
        S -= cnt;
        rem_strips -= cnt;
        if (S > 0 && w + 1 < workgroups) {             // the slab goes on in the next share
          ++w;
          k = 0;
          used = 0.0;
          budget = budget_now(S);
        }
      }
    }
  return longest;
}
inline int pass_share_pieces() { return RS_PIECES; }

// (test hook) all units of all queues in hand-out order; returns their number (may exceed cap)
inline int debug_pass_units(int batch, int nrb, int nch, int mode, int* out, int cap) {
  int total = 0;
  for (int g2 = 0; g2 < 8; ++g2) {
    const int cnt = rs_queue_count(g2, batch, nrb, nch, mode);
    for (int u = 0; u < cnt; ++u, ++total)
      if (total < cap) out[total] = rs_queue_unit(g2, u, batch, nrb, nch, mode);
  }
  return total;
}


// ---- step machinery -------------------------------------------------------------------------
inline int cap_for(int m) { return m <= 1 ? 1 : m <= 2 ? 2 : m <= 4 ? 4 : m <= 8 ? 8 : 16; }

// Rows per workgroup of k_flush: every wave re-reads its V strip (K x 1 KiB, from L2) per row block, so
// the block must be long where many ranks are pending, and short enough to give every CU several waves.
// Streaming launches with at least four 256-row workgroups per CU (big batches when k_flush is forced; N=8000): 256
// rows, tuned in round 1 (N=8000, 1 trajectory: 445 us against 488 us with 96 rows).
// Launches of several rounds of workgroups per CU: 96 rows.  Small launches leave the CUs with one to three workgroups
// each (two resident at a time) and the pass takes as long as the busiest CU, roughly (rows of a block) x (0.2 + load),
// load = workgroups per CU, rounded up to the next half where it is below that: the block height minimising it is
// taken.  N=2000, 1 trajectory: 80 rows (441 workgroups) 46 us, against 52 us with 96 rows (367) and 55 us with 64
// (543); N=500, 1 trajectory: 64 rows, 23 us against 30 us; N=2000, 2 / 4 / 6 trajectories (streaming): 96 rows 84 /
// 135 / 199 us against 108 / 164 / 208 us with 256 (profiles/r02_rows_per_block.txt).
inline int flush_workgroups(int n_hi, int rows_per_block) {
  const int gx = (n_hi + 255) / 256, gy = (n_hi + rows_per_block - 1) / rows_per_block;
  int total = 0;                                       // (the launcher's count: workgroups that reach the upper triangle)
  for (int by = 0; by < gy; ++by) total += std::max(0, gx - (by * rows_per_block) / 256);
  return total;
}
inline int flush_rows_per_block(const HostPlan* h, bool streaming, int n_hi) {
  if (h->opt_rows_per_block > 0) return (h->opt_rows_per_block + 15) / 16 * 16;
  const long cus = h->cu_count;
  if (streaming && (long)flush_workgroups(n_hi, 256) * h->batch >= 4 * cus) {
    // 256 rows, or 512 where that fills its rounds of 2 x CUs workgroups better (N=8000, 1 trajectory: 1024 workgroups
    // = two full rounds, 421 us against 454 us with 256 rows = 2016 workgroups; 2 trajectories 840 / 852 us)
    const long slots = 2 * cus;
    auto fill = [&](int r) {
      const long w = (long)flush_workgroups(n_hi, r) * h->batch;
      return (double)w / (double)((w + slots - 1) / slots * slots);
    };
    if ((long)flush_workgroups(n_hi, 512) * h->batch >= 2 * slots && fill(512) > fill(256) + 0.01) return 512;
    return 256;
  }
  if ((long)flush_workgroups(n_hi, 96) * h->batch > 5 * cus / 2) return 96;
  int best = 96;
  double best_cost = 0.0;
  for (int r = 64; r <= 256; r += 16) {
    const double load = (double)flush_workgroups(n_hi, r) * h->batch / (double)cus;
    const double cost = r * (0.2 + std::max(load, std::ceil(load) - 0.5));
    if (best_cost == 0.0 || cost < best_cost) {
      best_cost = cost;
      best = r;
    }
  }
  return best;
}

// The covariances of the batch stream through HBM when they cannot stay in the 256 MiB Infinity Cache.
inline bool streaming_pass(const HostPlan* h, int n_hi) {
  if (h->opt_streaming >= 0) return h->opt_streaming != 0;
  return (double)h->batch * 8.0 * n_hi * n_hi > 192.0e6;
}

// What the next covariance pass will launch (decided from the handle's state alone, so that the caller can ask before
// it launches).  `pending_k` ranks pending; `all_active`: as if every state index were active (the question "could a pass of
// this bank ever ...", asked before a run).
struct PassPlan {
  int n_hi, e_hi, nkt, kernel, rs_workgroups;
  bool streaming, long_few, beside;                    // beside: the row-slab pass leaves CUs free for a solve beside it
  int rows_per_block;                                  // (kernel 0) rows per workgroup of k_flush
  int rs_mode, rs_nch, rs_cs, rs_grid;                 // (kernel 2, on its work queues) hand-out (rs_queue_count) and workgroups launched
};
inline PassPlan plan_pass(const HostPlan* h, int pending_k, bool all_active = false) {
  PassPlan p{};
  p.n_hi = h->sizes_dirty ? h->n_max : *std::max_element(h->n.begin(), h->n.end());
  p.e_hi = 3;                                          // the grid covers the largest active bound of the batch
  for (int b = 0; b < h->batch; ++b) p.e_hi = std::max(p.e_hi, std::min(h->n[b], all_active ? h->n[b] : h->neff_enq[b]));
  if (h->sizes_dirty) p.e_hi = h->n_max;
  p.streaming = streaming_pass(h, p.n_hi);
  p.nkt = (pending_k + 3) / 4;
  p.kernel = h->opt_pass_kernel;
  p.rs_workgroups = h->opt_pass_workgroups > 0 ? std::min(h->opt_pass_workgroups, h->cu_count) : h->cu_count;
  // A few LONG trajectories (N = 8000 x 1: 126 slabs of up to 251 strips for 256 CUs): the row-slab pass with one equal
  // static share of the strips per workgroup (build_pass_shares) -- where a share is long enough (>= 40 strips) for
  // the pipeline fills at its piece boundaries not to matter.  The same for 10 .. 14 trajectories, where the queues
  // hold one to two whole slabs per workgroup and cannot balance them (N = 2000, 80 ranks, queues -> shares: x 10
  // 290 -> 261 us, x 11 321 -> 289, x 12 334 -> 303, x 13 350 -> 335, x 14 352 -> 346; N = 3000 x 12 753 -> 706;
  // 8, 9, 15 - 17 and from 23 on the queues are as good or better, 18 - 22 gain 2 - 5 % at N = 2000 but lose at N = 3000:
  // profiles/r03_pass_vs_batch.txt).
  const long slabs = (p.e_hi + 127) / 128, s_last = (p.e_hi - 1) >> 6;
  const long strips = (long)h->batch * (slabs * (s_last + 1) - slabs * (slabs - 1));
  p.long_few = (h->batch < 8 || (h->batch >= 10 && h->batch <= 14)) && h->opt_pass_chunk == 0 && strips >= 40L * p.rs_workgroups;
  // auto: the row-slab form where the batch streams through HBM and has at least one 128-row slab per CU (below
  // three per CU the slabs are cut into chunks of strips) or is a few long trajectories; measured at N=2000: 8
  // trajectories 256 us against 266 us with k_flush, 4 trajectories 166 / 164 us, 1 trajectory 97 / 52 us (pipeline
  // fills dominate)
  // SHORT slabs (n < 3000: fewer than 24 slabs of at most 47 strips) need more of them before the row-slab form's pipeline fills
  // are paid for -- 2.35 slabs per CU up to n = 2048, one per CU from n = 3072 on (N = 500 x 32, 64: the column strips +10 %, +3 %,
  // x 128: the row slabs +9 %; N = 1000 x 16, 32: strips +20 %, +7 %, x 64: slabs +2.5 %; N = 1500 x 16 and N = 2000 x 8: slabs
  // +4 %, +12 %; tools/mid_size_probe.sh, profiles/r04_n_sweep.txt)
  const double per_cu = slabs >= 24 ? 1.0 : slabs <= 16 ? 2.35 : 2.35 - (slabs - 16) * (1.35 / 8.0);
  if (p.kernel < 0)
    p.kernel = (p.streaming && ((double)h->batch * slabs >= per_cu * h->cu_count || p.long_few)) ? 2 : 0;
  // A few long trajectories on static shares: the pass leaves one CU per trajectory free, so that the next cadence's solve
  // (one workgroup per trajectory) can run beside it (the look-ahead of ekf_stream_run); always, not only when a solve
  // follows: the share table is built per workgroup count (N = 8000 x 1: 255 instead of 256 workgroups, 0.4 %).
  p.beside = p.kernel == 2 && p.long_few && h->batch < 8 && h->opt_lookahead && h->opt_pass_workgroups == 0 &&
             h->cu_count > 8 * h->batch;
  if (p.beside) p.rs_workgroups = h->cu_count - h->batch;
  if (p.kernel == 0) p.rows_per_block = flush_rows_per_block(h, p.streaming, p.e_hi);
  if (p.kernel != 2) return p;
  // Units of the work queues (the modes at rs_queue_count; equal static shares, where the pass takes them, replace them).
  // With an even number of trajectories per queue whole slabs taken trajectory by trajectory balance perfectly (16
  // trajectories: 366 us against 430 us in chunks of 22 strips); the last trajectory of an odd number finds no partner and
  // its slabs -- only they -- are cut in two (N=2000: 8 trajectories 203 us against 256 us with the former rule and 328 us
  // whole; 24: 557 us against 668 us); a batch that is no multiple of 8 would leave the queues with unequal work, so its
  // last trajectories are dealt over all queues slab by slab -- profiles/r02_chunk_sweep.txt, profiles/r02_batch_sweep.txt.
  // Below 8 trajectories (the row-slab kernel then only runs for long ones, N=8000) every slab is cut so that there are
  // about three units per CU.
  const int batch = h->batch, nrb = (p.e_hi + RS_ROWS - 1) / RS_ROWS, s_max = (p.e_hi + 63) / 64;   // strips of the longest slab
  int cs = s_max, nch = 1, mode = 0;
  if (h->opt_pass_chunk > 0) {                         // ("pass_chunk" option: every slab of every trajectory)
    cs = std::min(std::max(h->opt_pass_chunk, 1), s_max);
    nch = (s_max + cs - 1) / cs;
  } else if (batch >= 8) {
    if (batch % 8 == 0) {                              // pairs; an unpaired trajectory (8: each queue's only one) cut in two
      mode = 1;
      if (s_max >= 4) {
        cs = (s_max + 1) / 2;
        nch = 2;
      }
    } else if (batch <= 12 && s_max >= 8) {             // (N=2000: 9 trajectories 253 us against 329 us whole, 10: 284 / 333,
                                                       //  12: 327 / 342; 14: 360 / 344 -- from 13 on whole slabs)
      mode = 3;                                        // equal work per queue, half slabs, longest first
      nch = (s_max + 3) / 4;                           // h: half a chunk; chunks of cs = 2 h strips
      cs = 2 * nch;
    } else {
      mode = 2;                                        // equal work per queue, longest slabs first
    }
  } else {                                             // a few long trajectories (N=8000): about three units per CU
    long steps = 0;
    for (int rb = 0; rb < nrb; ++rb) steps += std::max(1, s_max - 2 * rb);
    steps *= batch;
    if ((long)nrb * batch < 3L * p.rs_workgroups) {
      cs = (int)std::max<long>(2, (steps + 3L * p.rs_workgroups - 1) / (3L * p.rs_workgroups));
      nch = (s_max + cs - 1) / cs;
    }
  }
  const long units = (long)nrb * (mode == 0 ? nch : mode == 3 ? 2 : 1) * batch;   // (modes 1, 2: at least; only the grid size depends on it)
  p.rs_mode = mode;
  p.rs_nch = nch;
  p.rs_cs = cs;
  p.rs_grid = (int)std::min<long>(p.rs_workgroups, units);
  return p;
}
inline PassPlan plan_pass(const HostPlan* h) { return plan_pass(h, h->pending_k); }
// The pending ranks as that pass would apply them: whole k-tiles (4 nkt).  What every kernel that reads P_base + W V takes.
inline int pending_kb(const HostPlan* h) { return (h->pending_k + 3) & ~3; }

// ---- the scaffold of the read-only queries and the log rings (ekf_api.hip: query_begin / query_end, ring_resize) ----
// Trajectories [b0, b0 + count) lie inside the bank (written so that no sum can overflow).
constexpr const char* BANK_RANGE_WHY = "trajectory range outside the bank";
inline bool bank_range_ok(const HostPlan* h, int b0, int count) { return b0 >= 0 && count > 0 && b0 <= h->batch - count; }

// Where a query's kernels write: the handle's staging buffer holds the `inputs` doubles the query uploads or uses as scratch,
// then one region per destination the device cannot write in place (ordinary host memory: copied back by query_end).  The site
// adds its destinations in order; plan_staging gives each no region -- absent, empty, or device-visible (pinned) -- or the
// next offset behind the ones before it, and returns the doubles the buffer must hold.  All sizes in doubles.
constexpr int STAGE_DSTS = 6;
struct StagingPlan {
  size_t inputs = 0;
  int ndst = 0;
  struct Dst { bool present, device, staged; size_t words, at; } dst[STAGE_DSTS];   // staged: region [at, at + words)
  void add(bool present, size_t words, bool device) { dst[ndst++] = Dst{present, device, false, words, 0}; }
};
inline size_t plan_staging(StagingPlan& s) {
  size_t total = s.inputs;
  for (int i = 0; i < s.ndst; ++i) {
    StagingPlan::Dst& d = s.dst[i];
    d.staged = d.present && d.words > 0 && !d.device;
    d.at = d.staged ? total : 0;
    total += d.staged ? d.words : 0;
  }
  return total;
}

// Steps [first, first + count) of a log are among the last `cap` of the `steps` logged ...
inline bool ring_range_ok(long long first, int count, long long steps, int cap) {
  return count >= 0 && first >= 0 && first <= steps - count && first >= steps - cap;
}
// ... and where they lie in its ring of `cap` rows: one piece, or two where the range wraps.  Piece i is `rows` ring rows from
// `slot` on, the range's steps from first + `done` on.
struct RingPieces { int n = 0; struct Piece { long slot, done, rows; } piece[2]; };
inline RingPieces ring_pieces(long long first, int count, int cap) {
  RingPieces r;
  for (long done = 0; done < count && r.n < 2; ++r.n) {   // (count <= cap: ring_range_ok)
    const long slot = (long)((first + done) % cap), rows = std::min<long>(count - done, cap - slot);
    r.piece[r.n] = {slot, done, rows};
    done += rows;
  }
  return r;
}

// ---- the per-step update (ekf_api.hip: enqueue_pass) ----
// Whether a step of this shape is run as one launch (the latency regime, see k_step_split): while every panel
// workgroup has a CU to itself.  N=2000: 1 trajectory 33.7 k steps/s against 28.0 k with two launches, 4 trajectories
// 79.2 k against 73.6 k, but 8 trajectories (504 panel workgroups) 85.8 k against 98.8 k.
inline bool step_is_split(int batch, int n_hi, int cus) { return (long)((n_hi + 63) / 64) * batch <= (long)cus; }
enum StepForm {
  STEP_PREDICT,        // prediction only, nothing pending: k_solve + k_predict_rc on rows / columns 0, 1 of P_base, O(n)
  STEP_SPLIT,          // one launch, the panels gathered beside the solve (k_step_split: few workgroups, the latency regime)
  STEP_SPLIT_TP,       // one launch in the throughput shape of the panels: workgroup 0 of a trajectory solves (k_panels_split)
  STEP_TWO,            // k_solve, then k_panels
};
struct StepPlan {
  int form, mcap;
  bool panels_latency;     // (STEP_TWO) k_panels<M, 4, true>: four waves split the pending ranks of 64 indices; else <M, 4, false>
  bool flush_before;       // the pending ranks are applied first: this step's would not fit behind them
};
inline StepPlan plan_step(const HostPlan* h, int m_hi, int n_hi) {
  StepPlan s{};
  s.mcap = cap_for(m_hi);
  s.panels_latency = (long)((n_hi + 63) / 64) * h->batch <= 512;
  if (m_hi == 0 && h->pending_k == 0) {
    s.form = STEP_PREDICT;
    return s;
  }
  // The kernels WRITE the rank slots of `mcap` landmarks behind the pending ones (zeros where a trajectory observes fewer) plus
  // the k-tile pad; the step is CHARGED the ranks of the busiest trajectory only (round 5: 2 per landmark, as the packed
  // cadences do) -- the next step starts right behind them and overwrites the zeros.  m = 5: 7 steps per pass (until round 4:
  // 5, the count rounded up to 8 landmarks), m = 12: 3 (2).
  s.flush_before = ((h->pending_k + ranks_for(s.mcap) + 3) & ~3) > KTOT;
  if (h->opt_fused_step && step_is_split(h->batch, n_hi, h->cu_count))
    s.form = STEP_SPLIT;
  else if (h->opt_fused_step && s.mcap <= 8 && !s.panels_latency && (long)(1 + (n_hi + 255) / 256) * h->batch <= 2L * h->cu_count)
    s.form = STEP_SPLIT_TP;   // (room left on the chip for one more workgroup per trajectory; 16 landmarks: registers for one wave per SIMD only)
  else
    s.form = STEP_TWO;
  return s;
}
// Behind a step that appended 2 m_hi ranks (pending_k / pending_steps count it): the cadence of the covariance pass -- a fixed
// number of steps if asked for, otherwise as many steps as fit `rank_limit` pending ranks (default 80): 5 steps at m = 8, 10 at
// m = 4, 40 at m = 1.
inline bool pass_due_after_step(const HostPlan* h, int m_hi) {
  const bool due = h->opt_flush_every > 0 ? h->pending_steps >= h->opt_flush_every
                                          : h->pending_k + std::max(2 * m_hi, 2) > h->opt_rank_limit;   // (a step like this one would not fit)
  return due || h->pending_k + 2 > KTOT;
}

// Which workgroup gets which static share.  build_pass_shares cuts the strips slab by slab, so consecutive shares are
// consecutive pieces of the same rows: at any time the workgroups of an XCD (equal blockIdx % 8) sit on 32 different
// column strips, every V strip they stage is used by one workgroup only, and V (80 ranks x ld doubles: 10 MB at N = 8000)
// does not fit an XCD's 4 MB L2 -- each of the 15 876 strip visits of a pass fetches its 40 KB from the Infinity Cache
// (650 MB per pass beside the 4.1 GB of P).  Workgroups advance at the same rate, so shares that START on the same column
// stay on the same column: the shares are sorted by (trajectory, first column) and dealt to the XCDs in runs, and the 32
// workgroups of an XCD walk (nearly) the same V strips together -- one fetch per XCD instead of one per workgroup.
inline void order_pass_shares(int workgroups, int pieces, int* table_ptr, size_t words) {
  std::vector<int> table(table_ptr, table_ptr + words);
  std::vector<int> order(workgroups);
  for (int w = 0; w < workgroups; ++w) order[w] = w;
  auto key = [&](int w) { return ((long)table[(size_t)w * pieces * 4] << 32) + table[(size_t)w * pieces * 4 + 2]; };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
  std::vector<int> slots;                              // blockIdx values XCD by XCD (workgroups go round-robin over the 8 XCDs)
  slots.reserve(workgroups);
  for (int x = 0; x < 8; ++x)
    for (int w = x; w < workgroups; w += 8) slots.push_back(w);
  std::vector<int> out(table.size(), 0);
  for (int q = 0; q < workgroups; ++q)
    std::copy_n(table.begin() + (size_t)order[q] * pieces * 4, (size_t)pieces * 4, out.begin() + (size_t)slots[q] * pieces * 4);
  std::copy(out.begin(), out.end(), table_ptr);
}

// ---- the packed cadences of ekf_stream_run (ekf_device.h: CadPlan) ----
// Steps [k, end) of the uploaded stream as a sequence of fused cadences, planned in one go.  Every trajectory walks its own
// flat sequence of predictions and landmark updates; a cadence gives it
//   * whole steps while their landmarks fit the slots that are left (steps that observe nothing are free),
//   * then, if slots are left and the next step does not fit, that step's prediction and as many of its landmarks as do fit
//     (the rest open the trajectory's next cadence -- no second prediction),
// within `slot_limit` landmark updates ("rank_limit" / 2, at most CAD_SLOTS) and `step_limit` touched steps ("flush_every",
// at most CAD_SLOTS: the kernels' per-step arrays).  The covariance pass follows every cadence but possibly the last, with
// as many ranks as the busiest trajectory appended (the others zero-fill): the number of passes of a run is what the
// trajectory with the most landmark updates needs at 40 per pass, however the counts are spread over steps and trajectories.
// A trajectory that has reached `end` idles (ns = 0).  The plan of a trajectory depends on its own observations only.
struct RunPlan {
  int ncad = 0;
  std::vector<CadPlan> entries;          // ncad x batch
  std::vector<int> slots_hi;             // per cadence: most landmark updates of any trajectory
  std::vector<int> steps_hi;             // per cadence: most steps completed by any trajectory
  std::vector<long> steps_sum;           // per cadence: steps completed, summed over the trajectories
};
inline int cadence_slot_limit(const HostPlan* h) { return std::max(1, std::min(CAD_SLOTS, h->opt_rank_limit / 2)); }
inline int cadence_step_limit(const HostPlan* h) { return h->opt_flush_every > 0 ? std::min(CAD_SLOTS, h->opt_flush_every) : CAD_SLOTS; }
inline bool cadences_possible(const HostPlan* h) {
  return h->opt_fused_cadence && h->pending_k == 0 && !h->sizes_dirty && (int)h->stream_m.size() == h->stream_steps * h->batch;
}
inline void plan_cadences(const HostPlan* h, int k, int end, RunPlan& rp) {
  const int B = h->batch, slot_limit = cadence_slot_limit(h), step_limit = cadence_step_limit(h);
  rp.ncad = 0;
  rp.entries.clear();
  rp.slots_hi.clear();
  rp.steps_hi.clear();
  rp.steps_sum.clear();
  std::vector<int> ct(B, k), cj(B, 0);   // cursor per trajectory: next step, next landmark of it (> 0: the step is cut)
  for (;;) {
    bool any = false;
    for (int b = 0; b < B; ++b) any = any || ct[b] < end;
    if (!any) break;
    const size_t base = rp.entries.size();
    rp.entries.resize(base + B);
    int slots_hi = 0, steps_hi = 0;
    long steps_sum = 0;
    for (int b = 0; b < B; ++b) {
      CadPlan& e = rp.entries[base + b];
      e = CadPlan{};
      e.t0 = ct[b];
      e.j0 = cj[b];
      int t = ct[b], j = cj[b], slots = 0, ns = 0, done = 0;
      e.jend = 0;
      while (t < end && ns < step_limit) {
        const int m = h->stream_m[(size_t)t * B + b], left = m - j;
        if (slots + left <= slot_limit) {              // the whole (rest of the) step
          slots += left;
          e.jend = m;
          ++ns;
          ++done;
          ++t;
          j = 0;
          continue;
        }
        const int room = slot_limit - slots;
        if (room > 0) {                                // cut: its prediction (if not yet done) and `room` landmarks
          slots += room;
          j += room;
          e.jend = j;
          ++ns;
        }
        break;
      }
      e.ns = ns;
      e.nslots = slots;
      const int t_last = ns > 0 ? e.t0 + ns - 1 : std::max(e.t0 - 1, 0);   // (an idle trajectory keeps its last step's bound)
      e.neff = std::min(h->n[b], std::max(h->floor_host[b], h->stream_own[(size_t)t_last * B + b]));
      ct[b] = t;
      cj[b] = j;
      slots_hi = std::max(slots_hi, slots);
      steps_hi = std::max(steps_hi, done);
      steps_sum += done;
    }
    rp.slots_hi.push_back(slots_hi);
    rp.steps_hi.push_back(steps_hi);
    rp.steps_sum.push_back(steps_sum);
    rp.ncad += 1;
  }
}

// ---- a fused cadence and what follows it (ekf_api.hip: enqueue_cadence, ekf_stream_run) ----
// Small launches, where the covariance pass leaves CUs free, run the next cadence's solve beside the pass (look-ahead) or chain
// the solves (see plan_cadence_launches).  Worth it where the pass is the column-strip kernel -- the row-slab pass fills every CU by
// itself -- and long enough to pay for the gather and the two cross-stream hand-overs, ~25 us together: from ~48 MB of
// covariance (LOOKAHEAD_MIN_MB; the chained order, whose hand-overs are counters instead of events, at every size: it wins at
// every size tried, N = 12 .. 1000, banks of 1 .. 32: +25 .. +43 %).  N = 2000 x 1: 38.7 k -> 45.1 k steps/s, x 2: 57.6 k ->
// 61.9 k, x 4: 89.5 k -> 92.1 k; N = 500 x 1 and N = 20 x 1 lose 4 - 9 %; N = 8000 x 1 on static shares, the pass on 255
// workgroups: 9.35 - 9.58 k -> 9.82 - 10.2 k
// ... or the row-slab pass on static shares that leaves the solves their CUs (a few long trajectories: N = 8000 x 1)
// ... and for banks of up to 40 trajectories: every solve workgroup has to find a CU beside the pass, and the gather grows with
// the bank (17 us at 32 trajectories, 71 us at 256) -- N = 500 x 32 +5 %, N = 300 x 48 -5 %, N = 200 x 128 -21 %,
// N = 100 x 256 -36 % with the look-ahead (bench.py --option lookahead=0; round 4)
constexpr int LOOKAHEAD_MIN_MB = 48;
inline bool beside_the_pass(const HostPlan* h, const PassPlan& plan) {
  const bool small_pass = plan.kernel == 0 && h->batch <= 40 &&
                          (h->opt_chain || (double)h->batch * 8.0 * plan.e_hi * plan.e_hi >= 1.0e6 * LOOKAHEAD_MIN_MB);
  const bool shares_pass = plan.kernel == 2 && (plan.beside || (plan.long_few && h->batch < 8 && h->opt_pass_workgroups > 0 &&
                                                                  h->opt_pass_workgroups + h->batch <= h->cu_count));
  return small_pass || shares_pass;
}
// Chained solves, decided per planned piece of a run (every solve of it then records its cadence's transform): banks of up to
// 40, as the look-ahead, and only where a pass of this bank can leave CUs to a solve beside it at all -- with every state index
// active and a full cadence pending (the headline's 32 x N = 2000 never does: its solves stay the plain instantiation).
inline bool plan_chain_run(const HostPlan* h, int ncad) {
  return h->opt_chain && h->opt_lookahead && ncad >= 2 && h->batch <= 40 && beside_the_pass(h, plan_pass(h, KTOT, true));
}
// Gather workgroups per trajectory of a chain launch: each counts itself off on the launch's gather counter.  (Every workgroup
// of the launch reserves the chain workgroup's LDS, a CU apiece: as many as leave the chip half free for what runs beside it.)
constexpr int CH_GW = 12;               // at most (12: a row of X and of P_0(C', C') per wave)
inline int chain_gather_workgroups(int batch, int cus) { return std::max(1, std::min(CH_GW, (cus / 2 - batch) / std::max(batch, 1))); }
// Panel launches of up to CAD_KS_WAVES waves of state indices (the latency regime) take the row-split form.
constexpr int CAD_KS_WAVES = 512;
inline bool panels_cad_latency_regime(int batch, int n_hi) { return (long)((n_hi + 63) / 64) * batch <= CAD_KS_WAVES; }
enum PanelForm {
  PANEL_TF,            // k_panels_cad_tf: chained cadences in the latency regime, the triangular-solve form
  PANEL_KS,            // k_panels_cad_ks: four waves split the rows of the panel of 64 state indices (the latency regime)
  PANEL_ONE,           // k_panels_cad<1>: one wave per workgroup (up to one wave per SIMD)
  PANEL_FOUR,          // k_panels_cad<4>
};
struct CadStepPlan {
  bool gather_cols;    // the solve's col_wgs extra workgroups gather the panel launch's mirrored column entries
  int col_wgs;
  bool due;            // the covariance pass follows the panel launch
  bool beside;         // ... beside the next cadence's solve (look-ahead)
  bool chain_next;     // ... and the next cadence's solve is chained to this one's
  bool w_from_v;       // the panel launch writes V only, the pass forms W from V
  int panel;           // PanelForm
};
// Cadence c of the run plan `rp` (neff_enq holding its active bounds); `presolved`: its solve has been enqueued already (chained
// / look-ahead).  The handle's pending ranks and steps are what the cadences before it left.
inline CadStepPlan plan_cadence_step(const HostPlan* h, const RunPlan& rp, int c, int n_hi, bool presolved) {
  CadStepPlan p{};
  // (the chain runs on one CU per trajectory: the rest of the chip gathers the panel launch's mirrored column entries meanwhile
  //  -- where there is a rest, and something to gather -- while its items, trajectories x strips of 64 state indices, are at
  //  most four rounds of the idle CUs' waves: N = 2000: up to ~80 trajectories; x 64 +1 - 2 %, x 128 -2 % on scattered
  //  landmarks, profiles/r05_scattered_indices.txt.  A solve launched beside a pass cannot: P_base is in motion.)
  const size_t cb_bytes = sizeof(double) * (size_t)h->batch * CAD_CU * h->ld;
  const long col_items = (long)h->batch * ((n_hi + 63) / 64), col_waves = 8L * (h->cu_count - h->batch);
  p.col_wgs = h->cu_count - h->batch;
  p.gather_cols = !presolved && h->opt_col_gather && cb_bytes <= ((size_t)1 << 30) && col_waves > 0 && col_items <= 4 * col_waves &&
                  rp.slots_hi[c] > 0;
  // the pass: behind every cadence but the run's last, and behind that one when its slots are used up
  const int ranks = 2 * rp.slots_hi[c];
  const bool more = c + 1 < rp.ncad;
  const int pend_after = h->pending_k + ranks, steps_after = h->pending_steps + rp.steps_hi[c];
  p.due = pend_after > 0 && (more || pend_after + 2 > std::min(KTOT, h->opt_rank_limit) ||
                             (h->opt_flush_every > 0 && steps_after >= h->opt_flush_every));
  p.beside = p.due && more && h->opt_lookahead && beside_the_pass(h, plan_pass(h, pend_after));
  p.chain_next = p.beside && h->chain_run;
  const bool latency = panels_cad_latency_regime(h->batch, n_hi);
  const long waves = (long)((n_hi + 63) / 64) * h->batch;
  if (p.chain_next && h->opt_panel_tform && !p.gather_cols && latency) p.panel = PANEL_TF;
  else if (h->opt_panel_shape > 0) p.panel = PANEL_KS + h->opt_panel_shape - 1;   // ("panel_shape": forced, diagnostics)
  else p.panel = latency ? PANEL_KS : (waves <= 1024 ? PANEL_ONE : PANEL_FOUR);
  // ("w_from_v") the pass follows this panel launch at once, nothing else is pending, both take the forms that know how
  p.w_from_v = h->opt_w_from_v && p.due && !p.beside && h->pending_k == 0 && ranks > 0 &&
               (p.panel == PANEL_ONE || p.panel == PANEL_FOUR) && plan_pass(h, pend_after).kernel == 2;
  return p;
}

// ---- a cadence's launches, in the order they are enqueued (ekf_api.hip: enqueue_cadence only executes the list) ----
// Cadence c of the run in flight (the run plan `rp`, uploaded): one solve launch, one panel launch; the covariance pass follows
// when it is due -- behind every cadence but the run's last, and behind that one when its slots are used up.
//
// Small launches, where the covariance pass leaves CUs free (the column-strip kernel on at least ~48 MB of covariance; the
// row-slab pass on static shares: a few long trajectories), do not run solve -> panel -> pass -> solve one behind the
// other: the only true dependency between two cadences of a trajectory is the sequential landmark recurrence
// (src/replay_no_ros.py:436-480: landmark j + 1 is linearised at the mean landmark j produced).  Three orders:
//   * SERIAL: [solve_c, log] -> panel_c -> pass_c where one is due and ranks are pending, all on the handle's stream.
//   * CHAINED SOLVES (round 6, "chain" = 1): every solve of the run also records the pose block behind its cadence
//     (k_solve_cad<true>: CadOut::posefin); k_chain_cad forms the next cadence's block and mean from the cadence's records and
//     from P_base as it stood BEFORE the cadence, so the handle's stream runs  solve_c -> chain_{c+1} -> solve_{c+1} -> ...  while
//     the second stream runs  gate -> panel_c -> pass_c -> mark -> gate -> ...  Hand-overs are device-scope counters (ekf_cadence.hip:
//     SYNC_*): the gate waits for solve_c (announced by chain_{c+1}'s start); panel_c ends when chain_{c+1}'s gather workgroups
//     have read what the pass rewrites and solve_{c+1} has been placed; chain_{c+1}'s gathers wait for the mark behind pass_{c-1}.
//     No event: a hand-over through the command processor costs the waiting stream 7 us behind a record and ~19 us across
//     streams (profiles/r06_chained_solves.txt); the counters cost a load.  Two copies of the records, of the pose rows (dprow3)
//     and of the inputs formed ahead (CadPre), used alternately.
//     A transition is ENQUEUED chain, solve, gate, panel, pass, mark: every device-side wait is for a launch that is already in
//     its queue (chain_{c+1}'s gathers: the previous transition's mark; panel_c: chain_{c+1}'s start and gathers, solve_{c+1}'s
//     start), so nothing can hang where the runtime maps both streams onto one hardware queue -- and the host calls nothing
//     that may block in between (every buffer exists before the cadence's first launch).  tests/host_plan_check.cpp
//     (check_cadence_orders) walks whole runs of these lists and checks exactly that.
//   * LOOK-AHEAD (round 3, "chain" = 0): panel_c -> k_gather_cad (the next block from P_base and the ranks still pending) ->
//     fork -> solve_{c+1} (first: it is ready to go the moment the gather ends, the pass has an event to wait for -- the one
//     workgroup per trajectory finds its CU before the pass fills the chip) | pass_c on the second stream -> join.
// `presolved` says that this cadence's solve has already been enqueued one of these ways; next_presolved that the next one's
// now is.  plan_cadence_step decides the flags (beside_the_pass where a pass leaves CUs to the next solve); this function turns
// them into the list and advances h->run.  The host's pending_k / pending_steps move where the list is executed: the PANEL op
// carries what it adds, the PASS clears them (flush_pending).
enum CadOpKind {
  OP_SOLVE, OP_LOG, OP_CHAIN, OP_GATE, OP_PANEL, OP_PASS, OP_MARK, OP_GATHER,
  OP_FORK,             // record ev_fork on the handle's stream, the second stream waits
  OP_JOIN,             // record ev_join on the second stream, the handle's waits
  OP_JOIN_AUX,         // the handle's stream waits for the chained passes in flight on the second (ev_pass)
};
enum CadStream { ON_MAIN, ON_AUX };                    // the handle's stream, its second stream
enum CadWhich { CAD_THIS = 0, CAD_NEXT = 1 };          // this cadence's buffers and plan row, or those of the one after it
struct CadOp {
  int kind = OP_SOLVE, stream = ON_MAIN;
  int which = CAD_THIS;    // (CHAIN reads this cadence's buffers whichever: `which` is the cadence whose block it forms)
  int cls = -1;            // profile class of its event pair: 1 solve, 2 chain / gather, 3 panel; 0 the pass (its own sampled pair); -1 none
  bool no_way_back = false;   // from this op on the next cadence's solve overwrites the pose mean and the pending-noise buffer:
                              // a failure cannot be undone (enqueue_cadence joins the streams and marks every trajectory undefined)
  bool sync = false;       // SOLVE, PANEL: takes part in the chained hand-overs (SOLVE: block and mean are the chain launch's)
  unsigned sigma = 0;      // CHAIN, GATE, MARK: the transition; SOLVE, PANEL: start_sigma
  unsigned target = 0;     // CHAIN: gather_target; PANEL: tail_target
  // SOLVE (SolveCadArgs)
  int gparts = 0;          // parts of the block in the block buffer (0: the solve gathers its block itself)
  bool chain = false;      // the instantiation that records the cadence's transform
  bool colbuf = false;     // SOLVE, PANEL: the mirrored column entries go through the column buffer
  int col_wgs = 0;
  // CHAIN (ChainArgs); pre_in also SOLVE: the copy of CadPre read / written, -1: none
  int pre_in = -1, pre_out = -1, gw = 1;
  bool wait_pass = false, plan2 = false;   // plan2: the plan row of the cadence after the next follows (for pre_out)
  // PANEL (PanelCadArgs), and what the host's pending counts become behind it
  int nrp = 0, form = 0, ranks = 0, steps_after = 0;
  bool skipw = false, keep_prow3 = false;
  int kb = 0;              // GATHER: the pending ranks in whole k-tiles
  bool wv = false;         // PASS: forms W from V
};
constexpr int CAD_OPS_MAX = 12;
struct CadLaunches {
  int n = 0;
  CadOp op[CAD_OPS_MAX];
  bool next_presolved = false;
  CadOp& add(int kind, int stream, int which, int cls) {
    CadOp& o = op[n++];
    o.kind = kind, o.stream = stream, o.which = which, o.cls = cls;
    return o;
  }
};
// `cp`: plan_cadence_step's answer for the same arguments (the caller has it: it decides which optional buffers must exist)
inline CadLaunches plan_cadence_launches(HostPlan* h, const RunPlan& rp, int c, int n_hi, bool presolved, const CadStepPlan& cp) {
  CadLaunches L;
  CadRun& r = h->run;
  const long serial = r.cad_serial++;                  // this cadence's number (CadPre copies are looked up by it)
  const int ranks = 2 * rp.slots_hi[c];                // every trajectory writes the busiest one's ranks (zeros beyond its own)
  const int pend_after = h->pending_k + ranks;
  auto join_aux = [&] {                                // whatever is still running on the second stream is waited for
    if (r.aux_pass) L.add(OP_JOIN_AUX, ON_MAIN, CAD_THIS, -1);
    r.aux_pass = false;
  };
  auto solve = [&](int which) -> CadOp& {
    CadOp& s = L.add(OP_SOLVE, ON_MAIN, which, 1);
    s.chain = h->chain_run;
    return s;
  };
  if (!presolved) {
    join_aux();
    CadOp& s = solve(CAD_THIS);
    s.colbuf = cp.gather_cols, s.col_wgs = cp.col_wgs;
    L.add(OP_LOG, ON_MAIN, CAD_THIS, -1);
  }
  CadOp panel;
  panel.kind = OP_PANEL, panel.cls = 3;
  panel.nrp = (ranks + 3) & ~3, panel.form = cp.panel, panel.skipw = cp.w_from_v, panel.colbuf = cp.gather_cols;
  panel.keep_prow3 = h->chain_run;                      // (only a chained run keeps the pose rows)
  panel.ranks = ranks;
  panel.steps_after = pend_after == 0 ? 0 : h->pending_steps + rp.steps_hi[c];   // (nothing observed anywhere in the bank: the panel launch applies the noise)
  if (cp.chain_next) {
    // the handle's stream: chain_{c+1} -> solve_{c+1}; the second stream: gate -> panel_c -> pass_c -> mark
    r.sigma += 1u;
    const int gw = h->chain_gw;
    r.gather_count += (unsigned)(h->batch * gw);
    CadOp& ch = L.add(OP_CHAIN, ON_MAIN, CAD_NEXT, 2);
    ch.sigma = r.sigma, ch.target = r.gather_count, ch.gw = gw, ch.wait_pass = r.aux_pass;
    // the next cadence's inputs if an earlier chain launch formed them; the one after it: formed by this launch
    ch.pre_in = r.pre_serial[(serial + 1) & 1] == serial + 1 ? (int)((serial + 1) & 1) : -1;
    ch.pre_out = c + 2 < rp.ncad ? (int)((serial + 2) & 1) : -1;
    ch.plan2 = ch.pre_out >= 0;
    if (ch.pre_out >= 0) r.pre_serial[ch.pre_out] = serial + 2;
    CadOp& s = solve(CAD_NEXT);                        // (block and mean from the chain launch: one part, no columns to gather)
    s.no_way_back = true;
    s.gparts = 1, s.chain = true, s.sync = true, s.sigma = r.sigma, s.pre_in = ch.pre_in;
    L.add(OP_LOG, ON_MAIN, CAD_NEXT, -1);              // (enqueued before the gate: it waits for nothing)
    // (a one-lane gate in front of the panel launch: ~5 us of the second stream, which has them to spare, and no workgroup of
    //  a large launch ever spins)
    L.add(OP_GATE, ON_AUX, CAD_THIS, -1).sigma = r.sigma;
    panel.stream = ON_AUX, panel.sync = true, panel.target = r.gather_count, panel.sigma = r.sigma;
  } else {
    join_aux();
  }
  L.op[L.n++] = panel;
  r.cpar ^= 1;
  r.cadences += 1;
  r.cadence_traj_steps += rp.steps_sum[c];
  if (cp.chain_next) {
    // pass_c behind the panel launch on the second stream, then the mark the next chain launch's gather workgroups wait for
    L.add(OP_PASS, ON_AUX, CAD_THIS, 0);
    L.add(OP_MARK, ON_AUX, CAD_THIS, -1).sigma = r.sigma;
    r.aux_pass = true;
    r.chained += 1;
    r.lookaheads += 1;
    L.next_presolved = true;
    return L;
  }
  if (pend_after == 0 || !cp.due) return L;
  if (!cp.beside) {
    if (cp.w_from_v) r.w_from_v_passes += 1;
    L.add(OP_PASS, ON_MAIN, CAD_THIS, 0).wv = cp.w_from_v;
    return L;
  }
  // look-ahead: gather (stream) -> { pass (second stream) | solve of the next cadence (stream) } -> join
  const int kb = (pend_after + 3) & ~3;                // (pending_kb behind the panel launch)
  L.add(OP_GATHER, ON_MAIN, CAD_NEXT, 2).kb = kb;
  L.add(OP_FORK, ON_MAIN, CAD_THIS, -1);
  CadOp& s = solve(CAD_NEXT);                          // (the block in the gather's parts; the mean is the handle's)
  s.no_way_back = true;
  s.gparts = (kb + 7) / 8;
  L.add(OP_LOG, ON_MAIN, CAD_NEXT, -1);
  L.add(OP_PASS, ON_AUX, CAD_THIS, 0);
  L.add(OP_JOIN, ON_AUX, CAD_THIS, -1);                // whatever follows on the handle's stream follows the pass
  r.lookaheads += 1;
  L.next_presolved = true;
  return L;
}
inline CadLaunches plan_cadence_launches(HostPlan* h, const RunPlan& rp, int c, int n_hi, bool presolved) {
  return plan_cadence_launches(h, rp, c, n_hi, presolved, plan_cadence_step(h, rp, c, n_hi, presolved));
}

// ---- the small-state path (ekf_small.hip): a filter bank whose covariances fit the LDS of a CU runs whole streams of steps per
// trajectory inside one workgroup, P resident in LDS; nothing is ever pending on it ----
inline int small_state_limit(int batch) { return batch >= SMALL_BANK_MIN ? SMALL_N_MAX_BANK : SMALL_N_MAX; }
inline bool small_path(const HostPlan* h) {
  return h->opt_small_state && h->n_max <= small_state_limit(h->batch) && h->pending_k == 0;
}
enum SmallForm {       // the kernel (ekf_small.hip) and its column tiles of 16
  SMALL_OCC_3,         // k_small_stream_occ<256, 3>: many small filters (more than three per CU), four waves per SIMD
  SMALL_3,             // k_small_stream<256, 3>
  SMALL_5,             // k_small_stream<256, 5>
  SMALL_TWO_7,         // k_small_stream_two<256, 7>: two workgroups per CU where LDS allows
  SMALL_9,             // k_small_stream<256, 9>
};
inline int plan_small(const HostPlan* h, int n_hi) {
  const int n = std::min(n_hi, SMALL_N_MAX_BANK);
  if (h->batch > 3 * h->cu_count && n <= 48) return SMALL_OCC_3;
  return n <= 48 ? SMALL_3 : n <= 80 ? SMALL_5 : n <= 112 ? SMALL_TWO_7 : SMALL_9;
}

// Validate one trajectory's whole observation list (all device passes of it) before any handle state changes:
// indices inside the current state, no index twice (the reference keys observations by landmark index,
// replay_no_ros.py:312-313).
// `unique` = false: an index may come twice (localisation on a frozen map, see plan_obs_lists).
// Returns nullptr when the list is good, else what is wrong with it.
inline const char* validate_obs(const HostPlan* h, int b, const int* idx, int m, std::vector<unsigned char>& seen, bool unique = true) {
  const int n_lm = (h->n[b] - 3) / 2;
  if (unique) seen.assign((size_t)std::max(n_lm, 1), 0);
  for (int i = 0; i < m; ++i) {
    const int id = idx[i];
    if (id < 0 || id >= n_lm) return "landmark index outside the current state (add_landmarks first)";
    if (!unique) continue;
    if (seen[id]) return "duplicate landmark index in one update (the reference keys observations by index, replay_no_ros.py:312-313)";
    seen[id] = 1;
  }
  return nullptr;
}

// ---- the observation lists of ekf_step / _update / _predict, ekf_localize_step / _update, and ekf_stream_upload per stream step ----
// One call's arguments checked before any handle state changes, in this order: lin / ang where the call predicts, m and the
// stride, every count in [0, stride], the observation arrays where anything is observed, every index inside its trajectory's map
// (validate_obs).  `unique`: SLAM refuses an index that comes twice in one trajectory's list; the frozen-map update is defined
// for it (the second observation is linearised at the pose the first one left, the landmark has not moved).  With the measurement
// model off neither counts nor lists are read.  m_hi: the most observations of any trajectory; more than MMAX of them run in
// `passes` device passes, the prediction in the first one only (fill_step cuts the list).  Returns nullptr, or what is wrong.
struct ObsPlan { int m_hi = 0, passes = 1; };
inline int loc_passes(int m_hi) { return std::max(1, (m_hi + MMAX - 1) / MMAX); }
inline const char* plan_obs_lists(const HostPlan* h, bool pred, bool upd, bool unique, const double* lin, const double* ang, const int* idx,
                                  const double* range, const double* bearing, const int* m, int stride, ObsPlan& op) {
  if (pred && (!lin || !ang)) return "NULL lin/ang";
  if (upd && (!m || stride < 0)) return "NULL m / bad stride";
  op.m_hi = 0;
  if (upd && h->cfg.enable_measurement_model)
    for (int b = 0; b < h->batch; ++b) {
      if (m[b] < 0 || m[b] > stride) return "m[b] must be in [0, stride]";
      op.m_hi = std::max(op.m_hi, m[b]);
    }
  if (op.m_hi > 0 && (!idx || !range || !bearing)) return "NULL observation arrays";
  if (op.m_hi > 0) {
    std::vector<unsigned char> seen;
    for (int b = 0; b < h->batch; ++b)
      if (const char* why = validate_obs(h, b, idx + (long)b * stride, m[b], seen, unique)) return why;
  }
  op.passes = loc_passes(op.m_hi);
  return nullptr;
}

// ---- the detection windows of ekf_step_detections and ekf_localize_detections: lin, ang, count and the stride; every count in
// [0, min(stride, EKF_DMAX)]; the detection arrays where anything is detected.  *m_hi: the most distinct tag ids of any window,
// capped at AMAX -- an upper bound of what the device matches (ignored, gated, unknown and bad ids count), the bound both entries
// select their kernels by; 0 with the measurement model off.  Returns nullptr, or what is wrong (then *m_hi is not written).
// One window of c detections, the w-th of arrays with `stride` detections per window; *distinct: its distinct tag ids, capped at AMAX.
inline const char* plan_det_window(int c, int stride, long w, const int* tag_id, const double* pose_t, const double* pose_err,
                                   int* distinct) {
  if (c < 0 || c > stride || c > DMAX) return "count must be <= min(stride, EKF_DMAX)";
  if (c > 0 && (!tag_id || !pose_t || !pose_err)) return "NULL detection arrays";
  const int* ids = c > 0 ? tag_id + w * stride : nullptr;
  int d = 0;
  for (int i = 0; i < c; ++i) d += std::find(ids, ids + i, ids[i]) == ids + i ? 1 : 0;
  *distinct = std::min(d, AMAX);
  return nullptr;
}
inline const char* plan_det_windows(const HostPlan* h, const double* lin, const double* ang, const int* count, const int* tag_id,
                                    const double* pose_t, const double* pose_err, int stride, int* m_hi) {
  if (!lin || !ang || !count || stride < 0) return "NULL array";
  int hi = 0;
  for (int b = 0; b < h->batch; ++b) {
    int distinct = 0;
    if (const char* why = plan_det_window(count[b], stride, b, tag_id, pose_t, pose_err, &distinct)) return why;
    hi = std::max(hi, distinct);
  }
  *m_hi = h->cfg.enable_measurement_model ? hi : 0;
  return nullptr;
}

// ekf_remove_landmarks (k_remove, ekf_remove.hip): the removal list of trajectories [b0, b0 + nb) checked -- every index
// inside every trajectory's landmark count, none twice, k >= 0 -- and turned into what the launch reads: src (new state index
// -> old) and dst (old -> new, -1 removed), one table for all of them (their sizes differ, the list does not), the first
// removed state index r0, the grid's rows (largest new size) and the columns per thread, nq (a whole row in registers).
struct RemovePlan {
  int k2 = 0, r0 = 0, rows = 0, nq = 0;
  std::vector<int> src, dst;
};
inline const char* plan_remove(const HostPlan* h, int b0, int nb, const int* lm, int k, RemovePlan& rp) {
  if (k < 0) return "ekf_remove_landmarks: k must be >= 0";
  if (k > 0 && !lm) return "ekf_remove_landmarks: NULL landmarks";
  int n_hi = 3, nl_lo = h->n[b0];
  for (int b = b0; b < b0 + nb; ++b) {
    n_hi = std::max(n_hi, h->n[b]);
    nl_lo = std::min(nl_lo, (h->n[b] - 3) / 2);
  }
  std::vector<unsigned char> gone((size_t)std::max(nl_lo, 1), 0);
  for (int i = 0; i < k; ++i) {
    if (lm[i] < 0 || lm[i] >= nl_lo) return "ekf_remove_landmarks: landmark index outside the state";
    if (gone[lm[i]]) return "ekf_remove_landmarks: landmark index given twice";
    gone[lm[i]] = 1;
  }
  rp.k2 = 2 * k;
  rp.src.assign((size_t)n_hi, 0);
  rp.dst.assign((size_t)n_hi, -1);
  rp.r0 = n_hi;
  int t = 0;
  for (int x = 0; x < n_hi; ++x) {
    const int l = (x - 3) >> 1;
    if (x >= 3 && l < nl_lo && gone[l]) {
      rp.r0 = std::min(rp.r0, x);
      continue;
    }
    rp.src[t] = x;
    rp.dst[x] = t++;
  }
  rp.rows = n_hi - rp.k2;
  rp.nq = 1;
  while (rp.nq < 64 && RM_THREADS * rp.nq < rp.rows) rp.nq *= 2;
  if (RM_THREADS * rp.nq < rp.rows) rp.nq = 96;        // (EKF_N_MAX_LIMIT <= 256 x 96)
  return nullptr;
}

// ---- the rank fronts (ekf_update_direct: k_direct, ekf_update_linear: k_linear; ekf_rank_front.h) ----
// the instantiation of a front kernel that serves `kpad` rows: the smallest compile-time row count that holds them (`full`:
// the kernel's own limit, DIRECT_ROWS or LINEAR_ROWS)
inline int front_rows_cap(int kpad, int full) { return kpad <= 4 ? 4 : kpad <= 8 ? 8 : kpad <= 16 ? 16 : full; }
// The table a front's launch reads and writes, ONE buffer of doubles for the whole bank of B trajectories: {`ints` ints per
// trajectory, rounded up to whole doubles | `dbls` doubles per trajectory | the results, NIS and applied per trajectory}.  Column
// 1 of every trajectory's ints is its active bound.  pack_direct / pack_linear fill the first two parts on the host.
struct FrontTable {
  size_t ints, dbls;
  size_t int_words(size_t B) const { return (B * ints + 1) / 2; }
  size_t words(size_t B) const { return int_words(B) + B * dbls + 2 * B; }
};

// ekf_update_direct (k_direct, ekf_direct.hip): the fixes of trajectories [b0, b0 + count) checked -- the range inside the
// bank, stride in 1..EKF_MMAX, m[bi] in 0..stride, every target a landmark of its trajectory's map or EKF_DIRECT_POSE /
// EKF_DIRECT_POSITION, no target twice and not both pose kinds in one trajectory, finite z, R and gate, gate > 0, every R block
// positive definite (leading minors of its upper triangle) -- and turned into the row plan: per trajectory of the range its
// D = sum of d stacked rows in the order given, the state index s of each row and where its measurement lives (4 * fix +
// component), and `kpad`, the largest D padded to a whole k-tile (what the covariance pass behind the launch applies).
// Returns nullptr, or what is wrong with the arguments (then nothing of `dp` is to be used).
struct DirectPlan {
  int kpad = 0;
  std::vector<int> D;              // count
  std::vector<int> s, src;         // count x DIRECT_ROWS (-1 / 0 beyond D)
};
inline int direct_rows(int target) { return target == EKF_DIRECT_POSE ? 3 : 2; }
inline const char* plan_direct(const HostPlan* h, int b0, int count, const int* target, const double* z, const double* R,
                               const int* m, int stride, const double* gate, DirectPlan& dp) {
  if (!bank_range_ok(h, b0, count)) return BANK_RANGE_WHY;
  if (stride < 1 || stride > MMAX) return "stride outside 1..EKF_MMAX";
  if (!target || !z || !R || !m) return "NULL target, z, R or m";
  dp.kpad = 0;
  dp.D.assign((size_t)count, 0);
  dp.s.assign((size_t)count * DIRECT_ROWS, -1);
  dp.src.assign((size_t)count * DIRECT_ROWS, 0);
  std::vector<int> seen;
  for (int bi = 0; bi < count; ++bi) {
    const int nl = (h->n[b0 + bi] - 3) / 2, mb = m[bi];
    if (mb < 0 || mb > stride) return "m[b] outside 0..stride";
    if (gate && !(gate[bi] > 0.0)) return "gate[b] must be > 0 (INFINITY: none) and not NaN";
    seen.clear();
    bool posed = false;
    int D = 0;
    for (int j = 0; j < mb; ++j) {
      const size_t f = (size_t)bi * stride + j;
      const int t = target[f], d = direct_rows(t);
      if (t < EKF_DIRECT_POSITION || t >= nl) return "target is neither a landmark of the trajectory's map nor a pose fix";
      if (t < 0) {
        if (posed) return "more than one pose / position fix in one trajectory";
        posed = true;
      } else {
        if (std::find(seen.begin(), seen.end(), t) != seen.end()) return "landmark target named twice in one trajectory";
        seen.push_back(t);
      }
      const double* zz = z + 3 * f;
      const double* rr = R + 9 * f;
      for (int a = 0; a < d; ++a) {
        if (!std::isfinite(zz[a])) return "non-finite z";
        for (int c = a; c < d; ++c)
          if (!std::isfinite(rr[3 * a + c])) return "non-finite R";
      }
      const double m2 = rr[0] * rr[4] - rr[1] * rr[1];
      bool pd = rr[0] > 0.0 && m2 > 0.0;
      if (pd && d == 3)
        pd = rr[0] * (rr[4] * rr[8] - rr[5] * rr[5]) - rr[1] * (rr[1] * rr[8] - rr[5] * rr[2]) + rr[2] * (rr[1] * rr[5] - rr[4] * rr[2]) > 0.0;
      if (!pd) return "an R block is not positive definite";
      if (D + d > DIRECT_ROWS) return "too many rows in one trajectory";
      for (int a = 0; a < d; ++a, ++D) {
        dp.s[(size_t)bi * DIRECT_ROWS + D] = t < 0 ? a : 3 + 2 * t + a;
        dp.src[(size_t)bi * DIRECT_ROWS + D] = 4 * j + a;
      }
    }
    dp.D[bi] = D;
    dp.kpad = std::max(dp.kpad, (D + 3) & ~3);
  }
  return nullptr;
}
// The host side of k_direct's table (ekf_device.h: DIRECT_INTS, DIRECT_DBLS) for the whole bank, from an accepted plan and the
// arrays it was made from: every trajectory its active bound and no row, those of the range their rows, fixes and gate.
inline FrontTable direct_table() { return FrontTable{DIRECT_INTS, DIRECT_DBLS}; }
inline void pack_direct(const HostPlan* h, const DirectPlan& dp, int b0, int count, const double* z, const double* R, const int* m,
                        int stride, const double* gate, std::vector<int>& ints, std::vector<double>& dbls) {
  const size_t B = (size_t)h->batch;
  ints.assign(B * DIRECT_INTS, 0);
  dbls.assign(B * DIRECT_DBLS, 0.0);
  for (size_t b = 0; b < B; ++b) {
    int* pi = ints.data() + b * DIRECT_INTS;
    pi[1] = h->opt_active_bound ? std::min(h->neff[b], h->n[b]) : h->n[b];
    for (int k = 0; k < DIRECT_ROWS; ++k) pi[2 + k] = -1;
  }
  for (int bi = 0; bi < count; ++bi) {
    int* pi = ints.data() + (size_t)(b0 + bi) * DIRECT_INTS;
    double* pd = dbls.data() + (size_t)(b0 + bi) * DIRECT_DBLS;
    pi[0] = dp.D[bi];
    std::copy_n(dp.s.data() + (size_t)bi * DIRECT_ROWS, DIRECT_ROWS, pi + 2);
    std::copy_n(dp.src.data() + (size_t)bi * DIRECT_ROWS, DIRECT_ROWS, pi + 2 + DIRECT_ROWS);
    std::copy_n(z + (size_t)bi * stride * 3, (size_t)m[bi] * 3, pd);
    std::copy_n(R + (size_t)bi * stride * 9, (size_t)m[bi] * 9, pd + 3 * MMAX);
    pd[DIRECT_DBLS - 2] = gate ? gate[bi] : INFINITY;
  }
}

// ekf_update_linear (k_linear, ekf_linear.hip): the measurements of trajectories [b0, b0 + count) checked -- the range inside
// the bank, lstride in 1..EKF_LINEAR_LMAX, dstride in 1..EKF_LINEAR_ROWS, k[bi] in 0..lstride, d[bi] in 0..dstride, every
// landmark inside its trajectory's map and none twice, finite H, r, R (what is read of them: the leading d rows, 3 + 2 k
// columns, R's upper triangle) and gate, gate > 0, every R positive definite (Cholesky of the upper triangle, on the host) --
// and turned into the plan: per trajectory of the range its row count D, sub-state size ns = 3 + 2 k, the state index of every
// sub-state entry in the order given, its highest landmark (-1: the pose alone; what the active bound has to cover), and
// `kpad`, the largest D padded to a whole k-tile (what the covariance pass behind the launch applies).
// Returns nullptr, or what is wrong with the arguments (then nothing of `lp` is to be used).
struct LinearPlan {
  int kpad = 0;
  std::vector<int> D, ns, lmax;    // count
  std::vector<int> s;              // count x LINEAR_NS (-1 beyond ns)
};
inline const char* plan_linear(const HostPlan* h, int b0, int count, const int* landmarks, const int* k, int lstride,
                               const double* H, const double* r, const double* R, const int* d, int dstride, const double* gate,
                               LinearPlan& lp) {
  if (!bank_range_ok(h, b0, count)) return BANK_RANGE_WHY;
  if (lstride < 1 || lstride > LINEAR_LMAX) return "lstride outside 1..EKF_LINEAR_LMAX";
  if (dstride < 1 || dstride > LINEAR_ROWS) return "dstride outside 1..EKF_LINEAR_ROWS";
  if (!landmarks || !k || !H || !r || !R || !d) return "NULL landmarks, k, H, r, R or d";
  const int nsl = 3 + 2 * lstride;
  lp.kpad = 0;
  lp.D.assign((size_t)count, 0);
  lp.ns.assign((size_t)count, 3);
  lp.lmax.assign((size_t)count, -1);
  lp.s.assign((size_t)count * LINEAR_NS, -1);
  double c[LINEAR_ROWS][LINEAR_ROWS];
  for (int bi = 0; bi < count; ++bi) {
    const int nl = (h->n[b0 + bi] - 3) / 2, kk = k[bi], D = d[bi];
    if (kk < 0 || kk > lstride) return "k[b] outside 0..lstride";
    if (D < 0 || D > dstride) return "d[b] outside 0..dstride";
    if (gate && !(gate[bi] > 0.0)) return "gate[b] must be > 0 (INFINITY: none) and not NaN";
    const int* lm = landmarks + (size_t)bi * lstride;
    int* s = lp.s.data() + (size_t)bi * LINEAR_NS;
    for (int a = 0; a < 3; ++a) s[a] = a;
    for (int p = 0; p < kk; ++p) {
      if (lm[p] < 0 || lm[p] >= nl) return "landmark index outside the trajectory's map";
      for (int q = 0; q < p; ++q)
        if (lm[q] == lm[p]) return "landmark index named twice in one trajectory";
      s[3 + 2 * p] = 3 + 2 * lm[p];
      s[4 + 2 * p] = 4 + 2 * lm[p];
      lp.lmax[bi] = std::max(lp.lmax[bi], lm[p]);
    }
    const int ns = 3 + 2 * kk;
    const double* Hb = H + (size_t)bi * dstride * nsl;
    const double* rb = r + (size_t)bi * dstride;
    const double* Rb = R + (size_t)bi * dstride * dstride;
    for (int a = 0; a < D; ++a) {
      if (!std::isfinite(rb[a])) return "non-finite r";
      for (int j = 0; j < ns; ++j)
        if (!std::isfinite(Hb[(size_t)a * nsl + j])) return "non-finite H";
      for (int q = a; q < D; ++q)
        if (!std::isfinite(Rb[(size_t)a * dstride + q])) return "non-finite R";
    }
    for (int j = 0; j < D; ++j) {                        // Cholesky of the upper triangle, lower factor in c
      double v = Rb[(size_t)j * dstride + j];
      for (int q = 0; q < j; ++q) v -= c[j][q] * c[j][q];
      if (!(v > 0.0) || !std::isfinite(v)) return "R is not positive definite";
      c[j][j] = std::sqrt(v);
      for (int a = j + 1; a < D; ++a) {
        double w = Rb[(size_t)j * dstride + a];
        for (int q = 0; q < j; ++q) w -= c[a][q] * c[j][q];
        c[a][j] = w / c[j][j];
      }
    }
    lp.D[bi] = D;
    lp.ns[bi] = ns;
    lp.kpad = std::max(lp.kpad, (D + 3) & ~3);
  }
  return nullptr;
}
// The host side of k_linear's table (ekf_device.h: LINEAR_INTS, linear_dbls) for the whole bank, packed by the launch's row cap
// `dp` and H's column count nsl = 3 + 2 * lstride, from an accepted plan and the arrays it was made from.  First the active
// bound (h->neff) of every trajectory that brings rows is raised over the highest landmark of its sub-state, as a landmark
// update of it would (fill_step): a general row correlates its targets.  Then every trajectory gets its bound, the pose as
// sub-state and no row, those of the range their sub-state, rows (H's leading ns columns, r, R's upper triangle) and gate.
inline FrontTable linear_table(int dp, int nsl) { return FrontTable{LINEAR_INTS, (size_t)linear_dbls(dp, nsl)}; }
inline void pack_linear(HostPlan* h, const LinearPlan& lp, int b0, int count, int lstride, const double* H, const double* r,
                        const double* R, int dstride, const double* gate, std::vector<int>& ints, std::vector<double>& dbls) {
  const size_t B = (size_t)h->batch;
  const int dp = front_rows_cap(lp.kpad, LINEAR_ROWS), nsl = 3 + 2 * lstride;
  const size_t per = (size_t)linear_dbls(dp, nsl);
  for (int bi = 0; bi < count; ++bi)
    if (lp.D[bi] > 0) h->neff[b0 + bi] = std::min(h->n[b0 + bi], std::max(h->neff[b0 + bi], 3 + 2 * (lp.lmax[bi] + 1)));
  ints.assign(B * LINEAR_INTS, 0);
  dbls.assign(B * per, 0.0);
  for (size_t b = 0; b < B; ++b) {
    int* pi = ints.data() + b * LINEAR_INTS;
    pi[1] = h->opt_active_bound ? std::min(h->neff[b], h->n[b]) : h->n[b];
    pi[2] = 3;
    for (int j = 0; j <= LINEAR_NS; ++j) pi[4 + j] = j < 3 ? j : -1;
  }
  for (int bi = 0; bi < count; ++bi) {
    int* pi = ints.data() + (size_t)(b0 + bi) * LINEAR_INTS;
    double* pd = dbls.data() + (size_t)(b0 + bi) * per;
    const int D = lp.D[bi], ns = lp.ns[bi];
    pi[0] = D;
    pi[2] = ns;
    std::copy_n(lp.s.data() + (size_t)bi * LINEAR_NS, LINEAR_NS, pi + 4);
    for (int a = 0; a < D; ++a) {
      std::copy_n(H + ((size_t)bi * dstride + a) * nsl, ns, pd + (size_t)a * nsl);
      pd[(size_t)dp * nsl + a] = r[(size_t)bi * dstride + a];
      for (int q = a; q < D; ++q) pd[(size_t)dp * nsl + dp + (size_t)a * dp + q] = R[((size_t)bi * dstride + a) * dstride + q];
    }
    pd[(size_t)dp * nsl + dp + (size_t)dp * dp] = gate ? gate[bi] : INFINITY;
  }
}

// ekf_predict_linear (k_predict_pose, ekf_predict_linear.hip): the inputs of trajectories [b0, b0 + count) checked -- the range
// inside the bank, pose, F and Q given, and for every APPLIED trajectory (apply == NULL: all) finite pose, F and Q (of Q what is
// read: the upper triangle) and a Q that is a covariance, possibly singular: no negative diagonal entry, q_ij^2 <= q_ii q_jj
// (plan_join's test for covT) and no negative determinant of the symmetrised upper triangle -- and turned into the launch's
// records (ekf_device.h: PredictIn), each with its trajectory's active bound capped by its size, plus `n_hi`, the largest bound
// of an applied trajectory (the grid; 0: nothing is applied).  An all-zero Q and a singular F are legal.
// Both singular tests allow for the rounding of their own arithmetic, so that a Q of rank 1 or 2 -- a a^T formed in floating
// point: q_ij^2 and q_ii q_jj then differ by a few roundings either way, and the determinant, exactly zero, comes out at
// +-1e-16 q_00 q_11 q_22 -- is not refused for it.  Pairwise: q_ij, q_ii and q_jj carry one rounding each, their products one
// more: "greater" means beyond q_ii q_jj (1 + 8 eps).  The determinant is a sum of six products of three entries, each at most
// q_00 q_11 q_22 in magnitude once the pairwise test has passed, ~12 roundings of that size: "negative" means below
// -32 eps q_00 q_11 q_22.
// Returns nullptr, or what is wrong with the arguments (then nothing of `pp` is to be used).
struct PredictPlan {
  int n_hi = 0;
  std::vector<PredictIn> rec;      // count
};
inline const char* plan_predict_linear(const HostPlan* h, int b0, int count, const double* pose, const double* F, const double* Q,
                                       const int* apply, PredictPlan& pp) {
  if (!bank_range_ok(h, b0, count)) return BANK_RANGE_WHY;
  if (!pose || !F || !Q) return "NULL pose, F or Q";
  constexpr double eps = 2.220446049250313e-16;
  pp.n_hi = 0;
  pp.rec.assign((size_t)count, PredictIn{});
  for (int bi = 0; bi < count; ++bi) {
    PredictIn& r = pp.rec[(size_t)bi];
    const int b = b0 + bi;
    r.apply = !apply || apply[bi] != 0;
    r.bound = h->opt_active_bound ? std::min(h->neff[b], h->n[b]) : h->n[b];
    if (!r.apply) continue;
    const double *p = pose + 3 * (size_t)bi, *f = F + 9 * (size_t)bi, *q = Q + 9 * (size_t)bi;
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(p[a])) return "non-finite pose";
      for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(f[3 * a + c])) return "non-finite F";
        if (c >= a && !std::isfinite(q[3 * a + c])) return "non-finite Q";
      }
    }
    for (int a = 0; a < 3; ++a) {
      if (q[4 * a] < 0.0) return "Q has a negative diagonal entry";
      for (int c = a + 1; c < 3; ++c)
        if (q[3 * a + c] * q[3 * a + c] > q[4 * a] * q[4 * c] * (1.0 + 8.0 * eps)) return "Q is not a covariance (q_ij^2 > q_ii q_jj)";
    }
    const double det = q[0] * (q[4] * q[8] - q[5] * q[5]) - q[1] * (q[1] * q[8] - q[5] * q[2]) + q[2] * (q[1] * q[5] - q[4] * q[2]);
    if (det < -32.0 * eps * q[0] * q[4] * q[8]) return "Q is not a covariance (negative determinant)";
    std::copy_n(p, 3, r.pose);
    std::copy_n(f, 9, r.F);
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) r.Q[3 * a + c] = q[3 * std::min(a, c) + std::max(a, c)];
    pp.n_hi = std::max(pp.n_hi, r.bound);
  }
  return nullptr;
}

// ---- localisation on a frozen map (ekf_localize_step / _update / _run: k_loc_solve + k_loc_rows, ekf_localize.hip) ----
// The arguments of a step are plan_obs_lists' with an index allowed TWICE in one call; each of its passes is two launches.
using LocPlan = ObsPlan;
inline const char* plan_localize(const HostPlan* h, bool pred, bool upd, const double* lin, const double* ang, const int* idx,
                                 const double* range, const double* bearing, const int* m, int stride, LocPlan& lp) {
  return plan_obs_lists(h, pred, upd, false, lin, ang, idx, range, bearing, m, stride, lp);
}
// The column groups of k_loc_rows' grid: LOC_THREADS columns each, up to the largest active bound a record of the launch can
// carry -- per trajectory the host's bound (which fill_step has raised over the call's landmarks) or the handle's floor,
// whichever is larger, and where `own` is given (a run: the stream's own bound per trajectory at the run's last step) that
// too; the whole state with the shortcut off or while the device has grown the sizes.
inline int loc_bound_hi(const HostPlan* h, const int* own = nullptr) {
  int hi = 3;
  for (int b = 0; b < h->batch; ++b) {
    int want = std::max(h->neff[b], h->floor_host[b]);
    if (own) want = std::max(want, own[b]);
    if (!h->opt_active_bound || h->sizes_dirty) want = h->sizes_dirty ? h->n_max : h->n[b];
    hi = std::max(hi, std::min(want, h->sizes_dirty ? h->n_max : h->n[b]));
  }
  return hi;
}
inline int loc_rows_groups(int n_hi) { return (std::max(n_hi, 3) + LOC_THREADS - 1) / LOC_THREADS; }

// ekf_localize_detections (k_loc_associate -> k_loc_solve -> k_loc_rows): the window checked by plan_det_windows, which gives
// m_hi, and what the call launches.  passes: a second k_loc_solve / k_loc_rows pair on the update-only records where m_hi > MMAX.
// groups: k_loc_rows' grid.  The device raises a trajectory's bound over the landmarks it matches, which the host does not know:
// where anything may be matched the grid covers the largest state (n_max while the sizes are dirty), else the bound mirrors as
// for the other localisation calls (loc_bound_hi); a workgroup beyond its trajectory's bound returns at once.
// Returns nullptr, or what is wrong (then nothing of `lp` is to be used and no handle state has changed).
struct LocDetPlan {
  int m_hi = 0, passes = 1, groups = 1;
};
inline const char* plan_localize_detections(const HostPlan* h, const double* lin, const double* ang, const int* count,
                                            const int* tag_id, const double* pose_t, const double* pose_err, int stride,
                                            LocDetPlan& lp) {
  int m_hi = 0;
  if (const char* why = plan_det_windows(h, lin, ang, count, tag_id, pose_t, pose_err, stride, &m_hi)) return why;
  lp.m_hi = m_hi;
  lp.passes = m_hi > MMAX ? 2 : 1;
  const int n_hi = h->sizes_dirty ? h->n_max : *std::max_element(h->n.begin(), h->n.end());
  lp.groups = loc_rows_groups(m_hi > 0 ? n_hi : loc_bound_hi(h));
  return nullptr;
}

// ---- the hypothesis bank (ekf_hyp_*: k_hyp_solve + k_hyp_rows, k_hyp_fill, k_hyp_compare, k_hyp_adopt; ekf_hypotheses.hip) ----
// What the planning functions read of a bank (ekf_hypotheses derives from this): the map's size and layout (the source handle's
// ld), the stride of a hypothesis's pose rows, the number of hypotheses, the map's active bound at creation (what a reset puts
// back) and an upper bound of every hypothesis's bound (the device raises them; this mirror only sizes k_hyp_rows' grid).
inline void fill_step(StepIn& s, int n_b, int& bound, double lin, double ang, int flags, const int* idx, const double* range,
                      const double* bearing, int m, int p);
struct HypBank {
  int device = 0, n = 0, ld = 0, ldx = 0, count = 0;
  long pstride = 0;
  ekf_config cfg{};
  int bound0 = 3, bound_hi = 3;
  // the uploaded stream (ekf_hypotheses_stream_upload; plan_hyp_stream): its steps, the records of a step and the stride between the
  // records k_hyp_solve reads, and per step the bound over the landmarks it names (3: none)
  int stream_steps = 0, stream_nrec = 1, stream_rec_stride = 0;
  std::vector<int> stream_bound;
  // a detection stream (ekf_hypotheses_detections_upload; plan_hyp_detection_stream): per step its update passes (1, or 2 where
  // it matched more than MMAX tags; empty: an index stream, one pass each) and the records between a step's first pass and its
  // second (k_hyp_associate's layout: the stream's steps)
  std::vector<int> stream_passes;
  size_t stream_pass_stride = 0;
  // whether the source slot had a tag table at creation (the bank's row of it: what a window of detections is walked against)
  bool has_tags = false;
  // the mixture log (ekf_hypotheses_log): the ring's rows (0: off) and the steps logged since it was switched on
  int log_cap = 0;
  long long log_steps = 0;
  // whether an unlabelled step has run (ekf_hypotheses_step_unlabelled / _update_unlabelled): the assignment rows hold its result
  bool unlabelled_run = false;
};
constexpr int HYP_COUNT_MAX = 1 << 16;                   // hypotheses of one bank (a grid dimension of the bank's launches)
// the bytes a hypothesis costs: its record, its three pose rows, its solve's record
inline size_t hyp_bytes_per(int ldx) { return sizeof(HypState) + 3 * sizeof(double) * (size_t)ldx + sizeof(LocRec); }
inline int hyp_fill_groups(int ldx) { return (std::max(ldx, 1) + HYP_THREADS - 1) / HYP_THREADS; }
inline int hyp_adopt_groups(int n) { return (std::max(n, 1) + HYP_THREADS - 1) / HYP_THREADS; }
inline int hyp_compare_groups(int n) { return (std::max(n, 1) + HYP_CMP_THREADS - 1) / HYP_CMP_THREADS; }
inline const char* plan_hyp_create(int n, int count) {
  if (count < 1 || count > HYP_COUNT_MAX) return "count must be in [1, 65536]";
  if (n < 3 || (n - 3) % 2 != 0) return "the source slot's size is not 3 + 2 N";
  return nullptr;
}
inline const char* plan_hyp_range(const HypBank* hy, int k0, int count) {
  if (k0 < 0 || count < 0 || k0 > hy->count || count > hy->count - k0) return "hypothesis range outside the bank";
  return nullptr;
}
// A step / an update of the bank checked as plan_localize checks a slot's -- in its order, an index may come twice -- with the two
// stride modes: motion_stride 0 = one (lin, ang) for every hypothesis, 1 = one each; obs_stride 0 = one list (m[0] observations at
// idx / range / bearing [0, m[0])) for every hypothesis, 1 = hypothesis k's m[k] observations at [k * stride, k * stride + m[k]).
// A list longer than EKF_MMAX is refused: the caller splits it into a step and update-only calls.  What the call launches: nrec
// records (one where both modes are 0, else one per hypothesis), rec_stride between the records k_hyp_solve reads, and
// k_hyp_rows' column groups up to bound_hi, the bank's bound raised over the highest landmark named.
// Returns nullptr, or what is wrong (then nothing of `hp` is to be used and nothing has changed).
struct HypStepPlan {
  int nrec = 1, rec_stride = 0, m_hi = 0, bound_hi = 3, groups = 1;
};
inline const char* plan_hyp_step(const HypBank* hy, bool pred, const double* lin, const double* ang, int motion_stride, const int* idx,
                                 const double* range, const double* bearing, const int* m, int stride, int obs_stride,
                                 HypStepPlan& hp) {
  if (pred && (!lin || !ang)) return "NULL lin/ang";
  if (pred && motion_stride != 0 && motion_stride != 1) return "motion_stride must be 0 (shared) or 1 (one per hypothesis)";
  if (!m || stride < 0) return "NULL m / bad stride";
  if (obs_stride != 0 && obs_stride != 1) return "obs_stride must be 0 (shared) or 1 (one list per hypothesis)";
  const int lists = obs_stride ? hy->count : 1;
  const bool meas = hy->cfg.enable_measurement_model != 0;
  hp.m_hi = 0;
  if (meas)
    for (int k = 0; k < lists; ++k) {
      if (m[k] < 0 || m[k] > stride) return "m[k] must be in [0, stride]";
      if (m[k] > MMAX) return "more than EKF_MMAX observations in one call: split the list into a step and update-only calls";
      hp.m_hi = std::max(hp.m_hi, m[k]);
    }
  if (hp.m_hi > 0 && (!idx || !range || !bearing)) return "NULL observation arrays";
  int id_hi = -1;
  if (hp.m_hi > 0) {
    const int n_lm = (hy->n - 3) / 2;
    for (int k = 0; k < lists; ++k)
      for (int i = 0; i < m[k]; ++i) {
        const int id = idx[(long)k * stride + i];
        if (id < 0 || id >= n_lm) return "landmark index outside the map";
        id_hi = std::max(id_hi, id);
      }
  }
  const bool per = (pred && motion_stride == 1) || obs_stride == 1;
  hp.nrec = per ? hy->count : 1;
  hp.rec_stride = per ? 1 : 0;
  hp.bound_hi = std::min(hy->n, std::max(hy->bound_hi, 3 + 2 * (id_hi + 1)));
  hp.groups = loc_rows_groups(hp.bound_hi);
  return nullptr;
}
// The hp.nrec records of a planned call (the bound travels on the device: StepIn::neff is not read)
inline void fill_hyp_records(const HypBank* hy, bool pred, const double* lin, const double* ang, int motion_stride, const int* idx,
                             const double* range, const double* bearing, const int* m, int stride, int obs_stride,
                             const HypStepPlan& hp, StepIn* out) {
  const bool meas = hy->cfg.enable_measurement_model != 0;
  for (int k = 0; k < hp.nrec; ++k) {
    const int km = pred ? k * motion_stride : 0, ko = k * obs_stride;
    const long off = (long)ko * stride;
    int unused = 3;
    fill_step(out[k], hy->n, unused, pred ? lin[km] : 0.0, pred ? ang[km] : 0.0, FLAG_UPDATE | (pred ? FLAG_PREDICT : 0),
              idx ? idx + off : nullptr, range ? range + off : nullptr, bearing ? bearing + off : nullptr, meas ? m[ko] : 0, 0);
  }
}
// ekf_hyp_reset's arguments: count poses and count 3 x 3 covariances (row-major; the upper triangle is read), finite, no negative
// variance; packs k_hyp_fill's count x 12 doubles into `init`.
inline const char* plan_hyp_reset(const HypBank* hy, int k0, int count, const double* pose, const double* cov, double* init) {
  if (const char* why = plan_hyp_range(hy, k0, count)) return why;
  if (count > 0 && (!pose || !cov)) return "NULL pose or cov";
  for (int i = 0; i < count; ++i)
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(pose[3 * (size_t)i + a])) return "non-finite pose";
      for (int c = a; c < 3; ++c)
        if (!std::isfinite(cov[9 * (size_t)i + 3 * a + c])) return "non-finite cov";
      if (cov[9 * (size_t)i + 4 * a] < 0.0) return "cov has a negative diagonal entry";
    }
  for (int i = 0; i < count; ++i) {
    std::copy_n(pose + 3 * (size_t)i, 3, init + 12 * (size_t)i);
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) init[12 * (size_t)i + 3 + 3 * a + c] = cov[9 * (size_t)i + 3 * std::min(a, c) + std::max(a, c)];
  }
  return nullptr;
}

// ekf_hypotheses_weigh / ekf_hypotheses_resample (k_hyp_weigh, k_hyp_plan: ONE workgroup of HYP_PLAN_THREADS, thread t on the
// records [t * chunk, (t + 1) * chunk); k_hyp_copy, k_hyp_split: grid (K, column groups) -- the hypothesis on x, so that K =
// 65536 is a legal grid --, a workgroup on HYP_COPY_COLS columns of one hypothesis's three rows).  u: the systematic resampler's
// offset in [0, 1); split: s in [0, 1), 0 = copies only; z: count x 3 standard normal draws, read where s > 0.  keep = 1 - s^2 is
// formed here, once.  Returns nullptr, or what is wrong (then nothing has changed).
inline int hyp_plan_chunk(int count) { return (std::max(count, 1) + HYP_PLAN_THREADS - 1) / HYP_PLAN_THREADS; }
inline int hyp_copy_groups(int ldx) { return (std::max(ldx, 1) + HYP_COPY_COLS - 1) / HYP_COPY_COLS; }
// the ints and doubles of scratch a bank's resampling keeps on the device: ancestors, offspring, surplus scan; weights
inline size_t hyp_resample_ints(int count) { return 3 * (size_t)count; }
struct HypResamplePlan {
  int chunk = 1, groups = 1;
  bool split = false;
  double u = 0.0, s = 0.0, keep = 1.0;
  // the device's gate (hyp_gate_open): plan, copy and split act where live > 0 and ess < ess_min.  +inf: wherever anything weighs
  double ess_min = std::numeric_limits<double>::infinity();
};
inline const char* plan_hyp_resample(const HypBank* hy, double u, double split, const double* z, HypResamplePlan& rp) {
  if (!(u >= 0.0 && u < 1.0)) return "u must be in [0, 1)";
  if (!(split >= 0.0 && split < 1.0)) return "split must be in [0, 1)";
  if (split > 0.0) {
    if (!z) return "split > 0 needs z (count x 3 standard normal draws)";
    for (size_t i = 0; i < 3 * (size_t)hy->count; ++i)
      if (!std::isfinite(z[i])) return "non-finite z";
  } else if (z) {
    return "z given with split == 0";
  }
  if (hy->count < 1 || hy->count > HYP_COUNT_MAX || hy->ldx < 2 || hy->ldx % 2 != 0) return "the bank's shape";
  rp.chunk = hyp_plan_chunk(hy->count);
  rp.groups = hyp_copy_groups(hy->ldx);
  rp.split = split > 0.0;
  rp.u = u;
  rp.s = split;
  rp.keep = 1.0 - split * split;
  return nullptr;
}

// ekf_hypotheses_stream_upload: ekf_hyp_step's arguments with a leading [step] axis -- lin / ang [steps] (motion_stride 0) or [steps][K];
// idx / range / bearing [steps][stride] and m [steps] (obs_stride 0) or [steps][K][stride] and [steps][K] -- every step checked by
// plan_hyp_step.  What the upload packs: nrec records per step (one where both strides are 0, else K), step s's at record
// s * nrec, and per step the bound over the landmarks it names, from which a run raises the bank's mirror.
// Returns nullptr, or what is wrong (then nothing of `sp` is to be used and nothing has changed).
struct HypStreamPlan {
  int steps = 0, nrec = 1, rec_stride = 0;
  std::vector<int> bound;
  size_t records() const { return (size_t)steps * (size_t)nrec; }
};
struct HypStreamArgs {                                   // one step's slices of the upload's arrays
  const double *lin, *ang;
  const int* idx;
  const double *range, *bearing;
  const int* m;
};
inline HypStreamArgs hyp_stream_step(const HypBank* hy, int s, const double* lin, const double* ang, int motion_stride, const int* idx,
                                     const double* range, const double* bearing, const int* m, int stride, int obs_stride) {
  const size_t mo = (size_t)s * (size_t)(motion_stride ? hy->count : 1), lists = (size_t)s * (size_t)(obs_stride ? hy->count : 1);
  const size_t oo = lists * (size_t)stride;
  return HypStreamArgs{lin + mo, ang + mo, idx ? idx + oo : nullptr, range ? range + oo : nullptr, bearing ? bearing + oo : nullptr,
                       m + lists};
}
inline const char* plan_hyp_stream(const HypBank* hy, int steps, const double* lin, const double* ang, int motion_stride,
                                   const int* idx, const double* range, const double* bearing, const int* m, int stride,
                                   int obs_stride, HypStreamPlan& sp) {
  if (steps < 0) return "steps must be >= 0";
  sp = HypStreamPlan{};
  if (steps == 0) return nullptr;                        // (frees the stream)
  if (!lin || !ang) return "NULL lin/ang";
  if (motion_stride != 0 && motion_stride != 1) return "motion_stride must be 0 (shared) or 1 (one per hypothesis)";
  if (!m || stride < 0) return "NULL m / bad stride";
  if (obs_stride != 0 && obs_stride != 1) return "obs_stride must be 0 (shared) or 1 (one list per hypothesis)";
  HypBank probe;                                         // the bank without its mirror: a step's own bound
  probe.n = hy->n;
  probe.count = hy->count;
  probe.cfg = hy->cfg;
  sp.bound.resize((size_t)steps);
  HypStepPlan hp;
  for (int s = 0; s < steps; ++s) {
    const HypStreamArgs a = hyp_stream_step(hy, s, lin, ang, motion_stride, idx, range, bearing, m, stride, obs_stride);
    if (const char* why = plan_hyp_step(&probe, true, a.lin, a.ang, motion_stride, a.idx, a.range, a.bearing, a.m, stride, obs_stride, hp))
      return why;
    sp.bound[(size_t)s] = hp.bound_hi;
  }
  sp.steps = steps;
  sp.nrec = hp.nrec;
  sp.rec_stride = hp.rec_stride;
  return nullptr;
}
// The sp.records() records of a planned upload, step s's from out[s * sp.nrec] on (fill_hyp_records')
inline void fill_hyp_stream(const HypBank* hy, const double* lin, const double* ang, int motion_stride, const int* idx,
                            const double* range, const double* bearing, const int* m, int stride, int obs_stride,
                            const HypStreamPlan& sp, StepIn* out) {
  HypStepPlan hp;
  hp.nrec = sp.nrec;
  hp.rec_stride = sp.rec_stride;
  for (int s = 0; s < sp.steps; ++s) {
    const HypStreamArgs a = hyp_stream_step(hy, s, lin, ang, motion_stride, idx, range, bearing, m, stride, obs_stride);
    fill_hyp_records(hy, true, a.lin, a.ang, motion_stride, a.idx, a.range, a.bearing, a.m, stride, obs_stride, hp,
                     out + (size_t)s * (size_t)sp.nrec);
  }
}
inline bool hyp_stream_loaded(const HypBank* hy) { return hy->stream_steps > 0; }

// ekf_hypotheses_run: steps [first, first + count) of the uploaded stream.  Per step k_hyp_solve + k_hyp_rows on the step's records
// (rec_offset) and, as the plan says: k_hyp_weigh (weigh: a resampling or the log needs the header), k_hyp_mixture into the
// log's next row (mixture: the log is on), k_hyp_plan + k_hyp_copy (resample: ess_fraction > 0) and k_hyp_split (rs.split).  The
// three resampling launches are gated on the device by rs.ess_min = ess_fraction * K, the double HypothesisBank.resample_if
// compares with; rs holds their shapes, the call sets rs.u per step.  groups[i]: k_hyp_rows' grid for step first + i, from the
// bank's mirror raised over the landmarks of the steps run so far; bound_hi: the mirror behind the run.
// u: count offsets in [0, 1), NULL iff ess_fraction == 0; z: count x K x 3 finite draws, NULL iff split == 0.
// Returns nullptr, or what is wrong (then nothing of `rp` is to be used and nothing has changed).
struct HypRunPlan {
  int first = 0, count = 0, nrec = 1, rec_stride = 0, bound_hi = 3;
  bool weigh = false, mixture = false, resample = false;
  HypResamplePlan rs;
  std::vector<int> groups;
  // a detection stream: step first + i runs passes[i] solve / rows pairs (an index stream: 1 each), pass p on the records at
  // rec_offset(i, p); weighing, the mixture row and the resampling follow the step's last pass
  std::vector<int> passes;
  size_t pass_stride = 0;
  size_t rec_offset(int i, int p = 0) const { return (size_t)(first + i) * (size_t)nrec + (size_t)p * pass_stride; }
};
inline const char* plan_hyp_run(const HypBank* hy, int first, int count, double ess_fraction, double split, const double* u,
                                const double* z, HypRunPlan& rp) {
  if (first < 0 || count < 0 || first > hy->stream_steps || count > hy->stream_steps - first) return "range outside the uploaded stream";
  if (!(ess_fraction >= 0.0) || !std::isfinite(ess_fraction)) return "ess_fraction must be finite and >= 0";
  if (!(split >= 0.0 && split < 1.0)) return "split must be in [0, 1)";
  if (split > 0.0 && ess_fraction == 0.0) return "split > 0 needs ess_fraction > 0: nothing is resampled";
  if (ess_fraction > 0.0) {
    if (!u) return "ess_fraction > 0 needs u (count offsets in [0, 1))";
    for (int i = 0; i < count; ++i)
      if (!(u[i] >= 0.0 && u[i] < 1.0)) return "u must be in [0, 1)";
  } else if (u) {
    return "u given with ess_fraction == 0";
  }
  if (split > 0.0) {
    if (!z) return "split > 0 needs z (count x K x 3 standard normal draws)";
    for (size_t i = 0; i < 3 * (size_t)count * (size_t)hy->count; ++i)
      if (!std::isfinite(z[i])) return "non-finite z";
  } else if (z) {
    return "z given with split == 0";
  }
  if (hy->count < 1 || hy->count > HYP_COUNT_MAX || hy->ldx < 2 || hy->ldx % 2 != 0) return "the bank's shape";
  rp = HypRunPlan{};
  rp.first = first;
  rp.count = count;
  rp.nrec = hy->stream_nrec;
  rp.rec_stride = hy->stream_rec_stride;
  rp.mixture = hy->log_cap > 0;
  rp.resample = ess_fraction > 0.0;
  rp.weigh = rp.resample || rp.mixture;
  rp.rs.chunk = hyp_plan_chunk(hy->count);
  rp.rs.groups = hyp_copy_groups(hy->ldx);
  rp.rs.split = split > 0.0;
  rp.rs.s = split;
  rp.rs.keep = 1.0 - split * split;
  rp.rs.ess_min = ess_fraction * (double)hy->count;
  rp.bound_hi = hy->bound_hi;
  rp.groups.resize((size_t)count);
  rp.passes.assign((size_t)count, 1);
  rp.pass_stride = hy->stream_pass_stride;
  for (int i = 0; i < count; ++i) {
    rp.bound_hi = std::min(hy->n, std::max(rp.bound_hi, hy->stream_bound[(size_t)(first + i)]));
    rp.groups[(size_t)i] = loc_rows_groups(rp.bound_hi);
    if (!hy->stream_passes.empty()) rp.passes[(size_t)i] = hy->stream_passes[(size_t)(first + i)];
  }
  return nullptr;
}

// ---- a bank's windows of raw detections (k_hyp_associate -> k_hyp_solve -> k_hyp_rows; ekf_loc_assoc.hip) ----
// ekf_hypotheses_step_detections: ONE window and ONE motion for every hypothesis, checked as plan_det_windows checks a window
// (plan_det_window), lin / ang finite.  m_hi: the window's distinct ids capped at AMAX -- an upper bound of what the device
// matches -- and 0 with the measurement model off; passes: a second k_hyp_solve / k_hyp_rows pair on the update-only record where
// m_hi > MMAX (a record that turns out empty leaves every hypothesis bit for bit: loc_solve_body's `apply`).  The device raises
// each hypothesis's bound over the landmarks it matched, which the host does not know: where anything may match, the mirror
// bound_hi becomes n and k_hyp_rows' grid covers the map -- a workgroup beyond its hypothesis's bound returns at once, no bit
// depends on the grid.  code: what a refusal returns -- EKF_ERR_STATE for a bank whose source slot had no tag table.
// Returns nullptr, or what is wrong (then nothing of `dp` but `code` is to be used and nothing has changed).
struct HypDetPlan {
  int m_hi = 0, passes = 1, bound_hi = 3, groups = 1, code = EKF_ERR_ARG;
};
inline const char* plan_hyp_detections(const HypBank* hy, double lin, double ang, int count, const int* tag_id, const double* pose_t,
                                       const double* pose_err, HypDetPlan& dp) {
  dp = HypDetPlan{};
  if (!hy->has_tags) {
    dp.code = EKF_ERR_STATE;
    return "the bank's source slot had no tag table (no ekf_step_detections / ekf_upload_tag_index before ekf_hyp_create)";
  }
  if (!std::isfinite(lin) || !std::isfinite(ang)) return "non-finite lin / ang";
  int distinct = 0;
  if (const char* why = plan_det_window(count, DMAX, 0, tag_id, pose_t, pose_err, &distinct)) return why;
  dp.m_hi = hy->cfg.enable_measurement_model ? distinct : 0;
  dp.passes = dp.m_hi > MMAX ? 2 : 1;
  dp.bound_hi = dp.m_hi > 0 ? hy->n : hy->bound_hi;
  dp.groups = loc_rows_groups(dp.bound_hi);
  return nullptr;
}
// ekf_hypotheses_detections_upload: `steps` windows -- lin / ang / count [steps], tag_id / pose_err [steps][stride], pose_t
// [steps][stride][3] --, every step checked as plan_hyp_detections checks its window.  What the upload holds: 2 * steps records
// in k_hyp_associate's layout (step s's first pass at record s, its second at steps + s).  bound / passes are exact and come
// from the device: finish_hyp_detection_stream, from the AssocOut records the association left.
struct HypDetStreamPlan {
  int steps = 0, code = EKF_ERR_ARG;
  std::vector<int> bound, passes;
  size_t records() const { return 2 * (size_t)steps; }
};
inline const char* plan_hyp_detection_stream(const HypBank* hy, int steps, const double* lin, const double* ang, const int* count,
                                             const int* tag_id, const double* pose_t, const double* pose_err, int stride,
                                             HypDetStreamPlan& sp) {
  sp = HypDetStreamPlan{};
  if (steps < 0) return "steps must be >= 0";
  if (steps == 0) return nullptr;                        // (frees the stream)
  if (!hy->has_tags) {
    sp.code = EKF_ERR_STATE;
    return "the bank's source slot had no tag table (no ekf_step_detections / ekf_upload_tag_index before ekf_hyp_create)";
  }
  if (!lin || !ang || !count || stride < 0) return "NULL array";
  for (int s = 0; s < steps; ++s) {
    if (!std::isfinite(lin[s]) || !std::isfinite(ang[s])) return "non-finite lin / ang";
    int distinct = 0;
    if (const char* why = plan_det_window(count[s], stride, s, tag_id, pose_t, pose_err, &distinct)) return why;
  }
  sp.steps = steps;
  return nullptr;
}
// The stream's exact shape from the association's records ao[0, steps): per step the bound over the landmarks it matched (3:
// none), as plan_hyp_stream gives an index stream's, and its passes.
inline void finish_hyp_detection_stream(const HypBank* hy, const AssocOut* ao, HypDetStreamPlan& sp) {
  sp.bound.assign((size_t)sp.steps, 3);
  sp.passes.assign((size_t)sp.steps, 1);
  const bool meas = hy->cfg.enable_measurement_model != 0;
  for (int s = 0; s < sp.steps; ++s) {
    const int m = meas ? std::max(0, std::min(ao[s].m, AMAX)) : 0;
    int id_hi = -1;
    for (int i = 0; i < m; ++i) id_hi = std::max(id_hi, ao[s].idx[i]);
    sp.bound[(size_t)s] = std::min(hy->n, std::max(3, 3 + 2 * (id_hi + 1)));
    sp.passes[(size_t)s] = m > MMAX ? 2 : 1;
  }
}
// ekf_hypotheses_download_tags: step -1 = the last single window (`single`: whether one has run), else a step of a detection stream
inline const char* plan_hyp_download_tags(const HypBank* hy, int step, bool single, int* code) {
  *code = EKF_ERR_ARG;
  if (step < -1) return "step must be -1 (the last single window) or a step of the uploaded detection stream";
  *code = EKF_ERR_STATE;
  if (step == -1) return single ? nullptr : "no window of detections has run (ekf_hypotheses_step_detections)";
  if (hy->stream_passes.empty() || step >= hy->stream_steps) return "no such step in an uploaded detection stream (ekf_hypotheses_detections_upload)";
  return nullptr;
}
// ---- a bank's unlabelled observations (k_hyp_score -> k_hyp_solve -> k_hyp_rows; ekf_hyp_assoc.hip) ----
// k_hyp_score's launch: one workgroup of HS_WAVES waves per hypothesis of the range; `chunks` chunks of HS_CHUNK landmarks cover
// the map and, where the query writes the full matrices, their `cap` columns (the columns beyond the map are NaN).
inline int hyp_score_chunks(int n, int cap) { return (std::max((n - 3) / 2, std::max(cap, 0)) + HS_CHUNK - 1) / HS_CHUNK; }
// ekf_hypotheses_associate: ONE list of m observations for hypotheses [k0, k0 + count).  cap_eff: the columns of the full
// matrices (0 without them).  Returns nullptr, or what is wrong (then nothing of `ap` is to be used and nothing has changed).
struct HypAssocPlan {
  int chunks = 0, cap_eff = 0;
};
inline const char* plan_hyp_associate(const HypBank* hy, int k0, int count, const double* range, const double* bearing, int m,
                                      const int* cand, const double* all_nis, const double* all_logdet, int cap, HypAssocPlan& ap) {
  ap = HypAssocPlan{};
  if (const char* why = plan_hyp_range(hy, k0, count)) return why;
  if (m < 0 || m > MMAX) return "m must lie in 0..EKF_MMAX";
  if (m > 0 && (!range || !bearing)) return "NULL observations";
  for (int q = 0; q < m; ++q)
    if (!std::isfinite(range[q]) || !std::isfinite(bearing[q])) return "non-finite observation";
  if (!cand) return "NULL cand";
  if ((all_nis == nullptr) != (all_logdet == nullptr)) return "all_nis and all_logdet are given together or not at all";
  if (all_nis && cap < (hy->n - 3) / 2) return "cap is below the map's landmark count";
  ap.cap_eff = all_nis ? cap : 0;
  ap.chunks = hyp_score_chunks(hy->n, ap.cap_eff);
  return nullptr;
}
// ekf_hypotheses_step_unlabelled (pred) / ekf_hypotheses_update_unlabelled: the motion as plan_hyp_step takes it, ONE list of m
// observations for every hypothesis, accept >= 0 (+inf: every candidate), miss finite.  m: the observations the launch scores --
// none while the measurement model is off, as ekf_hyp_update packs none --; chunks: k_hyp_score's; the host does not know what
// the device matches, so where anything may match the mirror bound_hi becomes n and k_hyp_rows' grid (groups) covers the map, as
// plan_hyp_detections has it.  Returns nullptr, or what is wrong (then nothing of `up` is to be used and nothing has changed).
struct HypUnlabelledPlan {
  int m = 0, chunks = 0, bound_hi = 3, groups = 1;
};
inline const char* plan_hyp_unlabelled(const HypBank* hy, bool pred, const double* lin, const double* ang, int motion_stride,
                                       const double* range, const double* bearing, int m, double accept, double miss,
                                       HypUnlabelledPlan& up) {
  up = HypUnlabelledPlan{};
  if (pred && (!lin || !ang)) return "NULL lin/ang";
  if (pred && motion_stride != 0 && motion_stride != 1) return "motion_stride must be 0 (shared) or 1 (one per hypothesis)";
  if (pred)
    for (int k = 0; k < (motion_stride ? hy->count : 1); ++k)
      if (!std::isfinite(lin[k]) || !std::isfinite(ang[k])) return "non-finite lin / ang";
  if (m < 0 || m > MMAX) return "m must lie in 0..EKF_MMAX";
  if (m > 0 && (!range || !bearing)) return "NULL observations";
  for (int q = 0; q < m; ++q)
    if (!std::isfinite(range[q]) || !std::isfinite(bearing[q])) return "non-finite observation";
  if (!(accept >= 0.0)) return "accept must be >= 0 (INFINITY: every candidate is accepted)";
  if (!std::isfinite(miss)) return "miss must be finite";
  up.m = hy->cfg.enable_measurement_model ? m : 0;
  up.chunks = hyp_score_chunks(hy->n, 0);
  up.bound_hi = up.m > 0 && hy->n > 3 ? hy->n : hy->bound_hi;
  up.groups = loc_rows_groups(up.bound_hi);
  return nullptr;
}
// ekf_hypotheses_download_assignment: rows [k0, k0 + count) of the last unlabelled step's assignment
inline const char* plan_hyp_assignment(const HypBank* hy, int k0, int count, const int* assign, int* code) {
  *code = EKF_ERR_ARG;
  if (const char* why = plan_hyp_range(hy, k0, count)) return why;
  if (count > 0 && !assign) return "NULL assign";
  *code = EKF_ERR_STATE;
  if (!hy->unlabelled_run) return "no unlabelled step has run (ekf_hypotheses_step_unlabelled / ekf_hypotheses_update_unlabelled)";
  return nullptr;
}

// ekf_hypotheses_log: a ring of `capacity` HypMixRow (0: off)
inline const char* plan_hyp_log(int capacity) {
  if (capacity < 0) return "capacity must be >= 0";
  if ((size_t)capacity * sizeof(HypMixRow) > ((size_t)1 << 36)) return "the ring would exceed 64 GiB";
  return nullptr;
}

// ekf_copy_trajectories (k_copy_traj, ekf_copy.hip): the k pairs (src_b[i] of `src` -> dst_b[i] of `dst`) checked -- indices
// inside their banks, no destination twice, inside one handle no trajectory both read and written, the same device, every
// source's size within the destination's n_max -- and grouped by source: a group is one source and up to COPY_FANOUT of its
// destinations (a workgroup loads a tile of the source once and stores it to each of them; a source with more destinations
// has several groups, so that a wide fork of small states still spreads over the chip).  The table the launch reads:
// COPY_GROUP_WORDS ints per group {source, first entry of its destinations, their number, the source's n}, then the
// destinations, `groups * COPY_GROUP_WORDS` on.  The sizes must be current (refresh_sizes) on both handles.
constexpr int COPY_FANOUT = 32;
constexpr int COPY_GROUP_WORDS = 4;
struct CopyPlan {
  int groups = 0, n_hi = 3;
  std::vector<int> tab;
};
inline const char* plan_copy(const HostPlan* dst, const int* dst_b, const HostPlan* src, const int* src_b, int k, CopyPlan& cp) {
  if (k < 0) return "ekf_copy_trajectories: k must be >= 0";
  if (k > 0 && (!dst_b || !src_b)) return "ekf_copy_trajectories: NULL index array";
  if (dst->device != src->device) return "ekf_copy_trajectories: the two handles are on different devices";
  std::vector<unsigned char> written((size_t)dst->batch, 0), read((size_t)src->batch, 0);
  for (int i = 0; i < k; ++i) {
    const int s = src_b[i], d = dst_b[i];
    if (s < 0 || s >= src->batch) return "ekf_copy_trajectories: source trajectory index out of range";
    if (d < 0 || d >= dst->batch) return "ekf_copy_trajectories: destination trajectory index out of range";
    if (written[d]) return "ekf_copy_trajectories: a destination trajectory is named twice";
    written[d] = 1;
    read[s] = 1;
    if (src->n[s] > dst->n_max) return "ekf_copy_trajectories: a source state is larger than the destination's n_max";
  }
  if (dst == src)
    for (int b = 0; b < dst->batch; ++b)
      if (written[b] && read[b]) return "ekf_copy_trajectories: inside one handle a trajectory cannot be both a source and a destination";
  std::vector<int> order((size_t)k);
  for (int i = 0; i < k; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return src_b[a] < src_b[b]; });
  std::vector<int> head, list;
  cp.n_hi = 3;
  for (int i = 0; i < k;) {
    const int s = src_b[order[i]];
    int cnt = 0;
    const int first = (int)list.size();
    while (i < k && src_b[order[i]] == s && cnt < COPY_FANOUT) {
      list.push_back(dst_b[order[i]]);
      ++i;
      ++cnt;
    }
    head.push_back(s);
    head.push_back(first);
    head.push_back(cnt);
    head.push_back(src->n[s]);
    cp.n_hi = std::max(cp.n_hi, src->n[s]);
  }
  cp.groups = (int)head.size() / COPY_GROUP_WORDS;
  cp.tab = head;
  cp.tab.insert(cp.tab.end(), list.begin(), list.end());
  return nullptr;
}
// tiles of 64 x 64 that reach the stored upper triangle of a state of size n (what k_copy_traj's grid enumerates)
inline int copy_tiles(int n) {
  const int t = (n + 63) / 64;
  return t * (t + 1) / 2;
}

// ekf_join_maps (k_join, ekf_join.hip): append the map of src_b[i] of `src` to trajectory dst_b[i] of `dst`.  The joined state is
// walked in ITEMS: item 0 is the pose (state indices 0..2), item q >= 1 landmark q - 1 (state indices 1 + 2 q, 2 + 2 q); with
// NA destination and NB source landmarks there are M = 1 + NA + NB items, the new ones from F = 1 + NA on.  A tile is
// JOIN_ITEMS x JOIN_ITEMS items (64 x 64 entries but for the pose's third row / column): whole 2 x 2 blocks, whatever the
// parity of their first column.  What a launch writes of the stored upper triangle: every entry whose COLUMN item is new, and
// in sequential mode (the destination's pose is replaced) every entry of the pose item's rows -- except the pose block itself,
// which the launch's extra workgroup writes with the mean and the size word.  join_tiles counts a pair's tiles, join_tile names
// tile t (row block ib <= column block jb): first the column blocks that hold a new item, block by block, then (sequential)
// row block 0 of the column blocks in front of them; join_writes says whether item pair (I, J) is written -- by the one tile
// that holds it.  Plain integer functions, the ones the kernel calls; tests/join_plan_check.cpp enumerates them.
constexpr int JOIN_ITEMS = 32;
constexpr int JOIN_PAIR_WORDS = 4;       // per pair {destination, source, NA, NB}
constexpr int JOIN_HEAD = 16;            // doubles in front of a pair's snapshot rows: g (3), pad, Sigma (3 x 3 row-major), pad
__host__ __device__ inline int join_tri(int x) { return x * (x + 1) / 2; }
__host__ __device__ inline int join_new_tiles(int NA, int NB) {
  return NB > 0 ? join_tri((NA + NB) / JOIN_ITEMS + 1) - join_tri((1 + NA) / JOIN_ITEMS) : 0;
}
__host__ __device__ inline int join_pose_tiles(int NA, int NB, bool seq) {
  return !seq ? 0 : NB > 0 ? (1 + NA) / JOIN_ITEMS : (NA + NB) / JOIN_ITEMS + 1;
}
__host__ __device__ inline int join_tiles(int NA, int NB, bool seq) { return join_new_tiles(NA, NB) + join_pose_tiles(NA, NB, seq); }
// tile t < join_tiles of a pair: its row block *ib and column block *jb
__host__ __device__ inline void join_tile(int NA, int NB, int t, int* ib, int* jb) {
  const int nn = join_new_tiles(NA, NB);
  if (t >= nn) {                                       // (sequential) the pose's rows over the kept landmarks
    *ib = 0;
    *jb = t - nn;
    return;
  }
  const int u = t + join_tri((1 + NA) / JOIN_ITEMS);
  int s = (int)((sqrtf(8.0f * (float)u + 1.0f) - 1.0f) * 0.5f);
  while (join_tri(s + 1) <= u) ++s;
  while (join_tri(s) > u) --s;
  *jb = s;
  *ib = u - join_tri(s);
}
// doubles of one pair's snapshot: the head, and in sequential mode the destination's three pose rows, ld apart
inline long join_snap_doubles(int ld, bool seq) { return JOIN_HEAD + (seq ? 3L * ld : 0L); }
// item pair (I, J), I <= J < M: does the launch's tile that holds it write it?
__host__ __device__ inline bool join_writes(int NA, int I, int J, bool seq) { return J > NA || (seq && I == 0 && J >= 1); }

// The k pairs checked -- indices inside their banks, no destination twice, inside one handle no trajectory both read and written,
// the same device, every joined size within the destination's n_max, T and covT both or neither, finite, covT (upper triangle) with
// a non-negative diagonal and c_ij^2 <= c_ii c_jj, twin_stride not below the largest NB where `twin` is given -- and turned into
// the launch's table (JOIN_PAIR_WORDS ints per pair, in the caller's order), the frames of the explicit mode (JOIN_HEAD doubles
// per pair: T, then covT mirrored from its upper triangle) and the grid: the most tiles of any pair, the largest NA and NB.
// The sizes must be current (refresh_sizes) on both handles.
struct JoinPlan {
  int pairs = 0, tiles_hi = 0, na_hi = 0, nb_hi = 0;
  bool seq = true;
  std::vector<int> tab;
  std::vector<double> frame;
};
inline const char* plan_join(const HostPlan* dst, const int* dst_b, const HostPlan* src, const int* src_b, int k, const double* T,
                             const double* covT, bool want_twin, int twin_stride, JoinPlan& jp) {
  if (k < 0) return "ekf_join_maps: k must be >= 0";
  if (k > 0 && (!dst_b || !src_b)) return "ekf_join_maps: NULL index array";
  if (dst->device != src->device) return "ekf_join_maps: the two handles are on different devices";
  if ((T == nullptr) != (covT == nullptr)) return "ekf_join_maps: T and covT must be given together";
  std::vector<unsigned char> written((size_t)dst->batch, 0), read((size_t)src->batch, 0);
  jp.pairs = k;
  jp.seq = T == nullptr;
  jp.tiles_hi = jp.na_hi = jp.nb_hi = 0;
  jp.tab.assign((size_t)k * JOIN_PAIR_WORDS, 0);
  jp.frame.assign(jp.seq ? 0 : (size_t)k * JOIN_HEAD, 0.0);
  for (int i = 0; i < k; ++i) {
    const int s = src_b[i], d = dst_b[i];
    if (s < 0 || s >= src->batch) return "ekf_join_maps: source trajectory index out of range";
    if (d < 0 || d >= dst->batch) return "ekf_join_maps: destination trajectory index out of range";
    if (written[d]) return "ekf_join_maps: a destination trajectory is named twice";
    written[d] = 1;
    read[s] = 1;
    const int NA = (dst->n[d] - 3) / 2, NB = (src->n[s] - 3) / 2;
    if ((long)dst->n[d] + 2L * NB > dst->n_max) return "ekf_join_maps: the joined state is larger than the destination's n_max";
    if (want_twin && twin_stride < NB) return "ekf_join_maps: twin_stride is below a source's landmark count";
    if (!jp.seq) {
      const double *t = T + 3 * (size_t)i, *c = covT + 9 * (size_t)i;
      double* f = jp.frame.data() + (size_t)i * JOIN_HEAD;
      for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(t[a])) return "ekf_join_maps: non-finite T";
        f[a] = t[a];
        for (int b = a; b < 3; ++b) {
          if (!std::isfinite(c[3 * a + b])) return "ekf_join_maps: non-finite covT";
          f[4 + 3 * a + b] = f[4 + 3 * b + a] = c[3 * a + b];
        }
      }
      for (int a = 0; a < 3; ++a) {
        if (c[4 * a] < 0.0) return "ekf_join_maps: covT has a negative diagonal entry";
        for (int b = a + 1; b < 3; ++b)
          if (c[3 * a + b] * c[3 * a + b] > c[4 * a] * c[4 * b]) return "ekf_join_maps: covT is not a covariance (c_ij^2 > c_ii c_jj)";
      }
    }
    int* w = jp.tab.data() + (size_t)i * JOIN_PAIR_WORDS;
    w[0] = d;
    w[1] = s;
    w[2] = NA;
    w[3] = NB;
    jp.tiles_hi = std::max(jp.tiles_hi, join_tiles(NA, NB, jp.seq));
    jp.na_hi = std::max(jp.na_hi, NA);
    jp.nb_hi = std::max(jp.nb_hi, NB);
  }
  if (dst == src)
    for (int b = 0; b < dst->batch; ++b)
      if (written[b] && read[b]) return "ekf_join_maps: inside one handle a trajectory cannot be both a source and a destination";
  return nullptr;
}

// ekf_transform (k_transform, ekf_transform.hip): move trajectories [b0, b0 + count) into another frame, in place.  The state is
// walked in k_join's items (item 0 the pose, item q landmark q - 1; M = 1 + N of them) and tiles of JOIN_ITEMS x JOIN_ITEMS
// items of the stored upper triangle.  Ma <= M items lie inside the active bound: an off-diagonal block whose column item is
// beyond it is an exact zero and stays one (R 0 R^T), so it is not visited; the diagonal blocks beyond the bound (the variances
// of never-observed landmarks) are.  With a frame covariance every item becomes correlated with every other: Ma = M.
// transform_tiles counts a trajectory's tiles: the triangle of the ta = ceil(Ma / JOIN_ITEMS) active tile columns, then the
// diagonal tiles of the tile columns behind them; transform_tile names tile t (row block ib <= column block jb);
// transform_writes says whether item pair (I, J), I <= J, is written -- by the one tile that holds it.  The pose block (0, 0)
// belongs to the launch's extra workgroup, with the means.  Plain integer functions, the ones the kernel calls;
// tests/transform_plan_check.cpp enumerates them.
constexpr int TF_WORDS = 4;              // per trajectory {trajectory, N, Ma, applied (0: T = 0 without a covariance -- nothing is touched)}
constexpr int TF_HEAD = 16;              // doubles of a trajectory's frame head: T (3), has-covariance, Sigma (3 x 3 row-major), pad
__host__ __device__ inline int transform_tile_cols(int items) { return (items + JOIN_ITEMS - 1) / JOIN_ITEMS; }
__host__ __device__ inline int transform_tiles(int M, int Ma) {
  const int ta = transform_tile_cols(Ma);
  return join_tri(ta) + (transform_tile_cols(M) - ta);
}
__host__ __device__ inline void transform_tile(int Ma, int t, int* ib, int* jb) {
  const int ta = transform_tile_cols(Ma), nt = join_tri(ta);
  if (t >= nt) {                                       // a diagonal tile beyond the active bound
    *ib = *jb = ta + (t - nt);
    return;
  }
  int s = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (join_tri(s + 1) <= t) ++s;
  while (join_tri(s) > t) --s;
  *jb = s;
  *ib = t - join_tri(s);
}
__host__ __device__ inline bool transform_writes(int Ma, int I, int J) { return J >= 1 && (I == J || J < Ma); }
// doubles per trajectory of the launch's frame buffer: its head (all heads first), and its means as they stood before the call
inline long transform_frame_doubles(int ld) { return TF_HEAD + (long)ld; }

// The call checked -- the range inside the bank (count == 0: nothing to do), T given and finite, cov NULL or per trajectory
// finite (of cov what is read: the upper triangle), with a non-negative diagonal, c_ij^2 <= c_ii c_jj (plan_join's test for covT)
// and no negative determinant (beyond its own rounding, as plan_predict_linear's Q) -- and turned into the launch's table
// (TF_WORDS ints per trajectory), the heads of the frame records (TF_HEAD doubles per trajectory: T, 1.0 where a covariance is
// given, the covariance mirrored from its upper triangle) and the grid: the most tiles of any applied trajectory.  The sizes
// must be current (refresh_sizes).  Returns nullptr, or what is wrong with the arguments.
struct TransformPlan {
  int tiles_hi = 0, applied = 0;
  bool with_cov = false;
  std::vector<int> tab;
  std::vector<double> head;
};
inline const char* plan_transform(const HostPlan* h, int b0, int count, const double* T, const double* cov, TransformPlan& tp) {
  if (count < 0) return "count must be >= 0";
  if (b0 < 0 || b0 > h->batch - count) return BANK_RANGE_WHY;
  if (count > 0 && !T) return "NULL T";
  constexpr double eps = 2.220446049250313e-16;
  tp.tiles_hi = tp.applied = 0;
  tp.with_cov = cov != nullptr;
  tp.tab.assign((size_t)count * TF_WORDS, 0);
  tp.head.assign((size_t)count * TF_HEAD, 0.0);
  for (int bi = 0; bi < count; ++bi) {
    const int b = b0 + bi;
    const double* t = T + 3 * (size_t)bi;
    double* f = tp.head.data() + (size_t)bi * TF_HEAD;
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(t[a])) return "non-finite T";
      f[a] = t[a];
    }
    if (cov) {
      const double* c = cov + 9 * (size_t)bi;
      for (int a = 0; a < 3; ++a)
        for (int d = a; d < 3; ++d) {
          if (!std::isfinite(c[3 * a + d])) return "non-finite cov";
          f[4 + 3 * a + d] = f[4 + 3 * d + a] = c[3 * a + d];
        }
      for (int a = 0; a < 3; ++a) {
        if (c[4 * a] < 0.0) return "cov has a negative diagonal entry";
        for (int d = a + 1; d < 3; ++d)
          if (c[3 * a + d] * c[3 * a + d] > c[4 * a] * c[4 * d]) return "cov is not a covariance (c_ij^2 > c_ii c_jj)";
      }
      const double det = c[0] * (c[4] * c[8] - c[5] * c[5]) - c[1] * (c[1] * c[8] - c[5] * c[2]) + c[2] * (c[1] * c[5] - c[4] * c[2]);
      if (det < -32.0 * eps * c[0] * c[4] * c[8]) return "cov is not a covariance (negative determinant)";
      f[3] = 1.0;
    }
    const int N = (h->n[b] - 3) / 2, M = 1 + N;
    const int bound = h->opt_active_bound ? std::max(3, std::min(h->neff[b], h->n[b])) : h->n[b];
    const int Ma = cov ? M : std::min(M, 1 + (bound - 3 + 1) / 2);
    const bool applied = cov || t[0] != 0.0 || t[1] != 0.0 || t[2] != 0.0;
    int* w = tp.tab.data() + (size_t)bi * TF_WORDS;
    w[0] = b;
    w[1] = N;
    w[2] = Ma;
    w[3] = applied ? 1 : 0;
    if (applied) {
      tp.applied += 1;
      tp.tiles_hi = std::max(tp.tiles_hi, transform_tiles(M, Ma));
    }
  }
  if (tp.tiles_hi + 1 > 65535) return "the state is too large for one launch";
  return nullptr;
}

// ekf_associate (k_assoc_query / k_assoc_finish, ekf_associate.hip): the launch shape of the query over trajectories
// [b0, b0 + count).  lane = landmark, a workgroup per chunk of AQ_CHUNK landmarks and trajectory, as k_marginals: N = 2000 x 1 is
// 32 workgroups on 32 CUs, 32 x N = 2000 is 1024 (four per CU of 256), N = 20 x 256 one per trajectory.  The grid covers the
// largest landmark count of the range -- or `cap`, where the full matrices are asked for (their NaN padding is written by the
// workgroups beyond a trajectory's landmarks) -- and at least one chunk, so that every observation gets a record.
struct AssocQueryPlan {
  int nl_hi;           // largest landmark count of the range
  int chunks;          // grid.x; grid.y = count
};
inline AssocQueryPlan plan_assoc_query(const HostPlan* h, int b0, int count, int cap) {
  AssocQueryPlan p{};
  for (int b = b0; b < b0 + count; ++b) p.nl_hi = std::max(p.nl_hi, (h->n[b] - 3) / 2);
  p.chunks = std::max(1, (std::max(p.nl_hi, cap) + AQ_CHUNK - 1) / AQ_CHUNK);
  return p;
}

// ekf_download_joint (k_joint, ekf_joint.hip): validates the selections of trajectories [b0, b0 + count) -- k[bi] <= stride
// landmarks each, in any order -- and decides the launch: a workgroup per (trajectory, JQ_TILE x JQ_TILE tile of the upper
// triangle of the ns x ns sub-matrix), ns = 3 + 2 stride: 15 tiles at stride = EKF_JMAX, 480 workgroups for a bank of 32, one
// at stride <= 14.  `sel` becomes what the kernel reads, per trajectory 2 * nsp ints (nsp = ns rounded up to whole tiles): the
// sub-state SORTED by state index -- the stored upper triangle of P is then the upper triangle of the sub-matrix -- as
// sidx[t], the state index of sorted entry t, and spos[t], its row / column of the output.  Entries beyond a trajectory's own
// 3 + 2 k[bi] are sidx = -1 with spos = t (NaN rows and columns), the padding beyond ns is spos = -1 (never written).
// Returns nullptr, or what is wrong with the arguments (then nothing of `jp` or `sel` is to be used).
struct JointQueryPlan {
  int ns;              // rows / columns of one trajectory's output
  int nt;              // tiles per row of the sub-matrix
  int tiles;           // grid.x = nt (nt + 1) / 2; grid.y = count
  int nsp;             // nt * JQ_TILE
};
inline const char* plan_joint_query(const HostPlan* h, int b0, int count, const int* landmarks, const int* k, int stride,
                                    JointQueryPlan& jp, std::vector<int>& sel, std::vector<std::pair<int, int>>& order) {
  if (!bank_range_ok(h, b0, count)) return BANK_RANGE_WHY;
  if (stride < 1 || stride > JMAX) return "stride outside 1..EKF_JMAX";
  if (!landmarks || !k) return "NULL landmarks or k";
  jp.ns = 3 + 2 * stride;
  jp.nt = (jp.ns + JQ_TILE - 1) / JQ_TILE;
  jp.tiles = jp.nt * (jp.nt + 1) / 2;
  jp.nsp = jp.nt * JQ_TILE;
  sel.assign((size_t)count * 2 * jp.nsp, -1);
  for (int bi = 0; bi < count; ++bi) {
    const int nl = (h->n[b0 + bi] - 3) / 2, kk = k[bi];
    if (kk < 0 || kk > stride) return "k[b] outside 0..stride";
    const int* lm = landmarks + (size_t)bi * stride;
    order.clear();                                     // (landmark, its place in the selection)
    for (int p = 0; p < kk; ++p) {
      if (lm[p] < 0 || lm[p] >= nl) return "landmark index outside the state";
      order.emplace_back(lm[p], p);
    }
    std::sort(order.begin(), order.end());
    for (int p = 1; p < kk; ++p)
      if (order[p].first == order[p - 1].first) return "landmark index named twice";
    int* sidx = sel.data() + (size_t)bi * 2 * jp.nsp;
    int* spos = sidx + jp.nsp;
    for (int a = 0; a < 3; ++a) sidx[a] = spos[a] = a;
    for (int p = 0; p < kk; ++p)
      for (int d = 0; d < 2; ++d) {
        sidx[3 + 2 * p + d] = 3 + 2 * order[p].first + d;
        spos[3 + 2 * p + d] = 3 + 2 * order[p].second + d;
      }
    for (int t = 3 + 2 * kk; t < jp.ns; ++t) spos[t] = t;
  }
  return nullptr;
}

// ekf_factor (ekf_factor.hip): the blocked Cholesky factorisation of trajectories [b0, b0 + count) and what is kept of it.
// The workspace holds count matrices of lw x lw doubles, lw = the range's largest n rounded up to whole blocks of FB; all of
// its arithmetic is size_t (n_max = 21823 x 32 trajectories is 122 GB: beyond every 32-bit count, and refused by the
// allocation, not by an overflow).  Block step k of nblk launches the diagonal block (count workgroups), the row panel
// (factor_panel_groups x count) and the trailing down-date (t (t + 1) / 2 x count, t = factor_trail_tiles_per_row):
// 3 nblk - 2 launches behind the load, 188 at n = 4003.  ekf_factor_solve is 2 nblk - 1 launches (the block's substitution, the
// update of the columns to its right), ekf_factor_multiply one.
struct FactorPlan {
  int n_hi;            // largest state of the range
  int nblk;            // its blocks
  int lw;              // row stride of the workspace (doubles)
  size_t tstride;      // trajectory stride (doubles)
  size_t words;        // doubles of the whole workspace
  long launches;       // kernel launches of the factorisation
};
// column groups of 256 (a thread per column) of block step k's row panel; 0: the last block has none
inline int factor_panel_groups(int nblk, int k) { return ((nblk - k - 1) * FB + 255) / 256; }
// 128 x 128 tiles per row of block step k's trailing triangle (two blocks each; the last one may hold a single block)
inline int factor_trail_tiles_per_row(int nblk, int k) { return (nblk - k - 1 + 1) / 2; }
inline const char* plan_factor(const HostPlan* h, int b0, int count, FactorPlan& fp) {
  if (!bank_range_ok(h, b0, count)) return BANK_RANGE_WHY;
  fp.n_hi = 0;
  for (int b = b0; b < b0 + count; ++b) fp.n_hi = std::max(fp.n_hi, h->n[b]);
  fp.nblk = (fp.n_hi + FB - 1) / FB;
  fp.lw = fp.nblk * FB;
  fp.tstride = (size_t)fp.lw * (size_t)fp.lw;
  fp.words = fp.tstride * (size_t)count;
  fp.launches = 1 + (fp.nblk > 0 ? 3L * fp.nblk - 2 : 0);
  return nullptr;
}
// The factor a handle holds: the range and each trajectory's n and info at the time of ekf_factor.
struct FactorHeld {
  bool held = false;
  int b0 = 0, count = 0, lw = 0;
  size_t tstride = 0;
  std::vector<int> n, info;
};
// ekf_factor_solve / ekf_factor_multiply on trajectories [b0, b0 + count): the arguments (a message: EKF_ERR_ARG), then the
// factor (*state = true: EKF_ERR_STATE).  x: count x nrhs x stride, of which the first n of every column must be finite.
// *nblk_hi: blocks of the range's largest factored state.
constexpr int FACTOR_STRIDE_MAX = 1 << 20;
inline const char* plan_factor_apply(const HostPlan* h, const FactorHeld& fh, int b0, int count, const double* x, int nrhs, int stride,
                                     bool* state, int* nblk_hi) {
  *state = false;
  if (!bank_range_ok(h, b0, count)) return BANK_RANGE_WHY;
  if (!x) return "NULL right-hand sides";
  if (nrhs < 1 || nrhs > FACTOR_RHS) return "nrhs outside 1..EKF_FACTOR_RHS";
  if (stride < 1 || stride > FACTOR_STRIDE_MAX) return "stride out of bounds";
  *state = true;
  if (!fh.held) return "no factor is held (ekf_factor)";
  if (b0 < fh.b0 || b0 - fh.b0 > fh.count - count) return "trajectory range outside the factored one";
  *state = false;
  int n_hi = 0;
  for (int bi = 0; bi < count; ++bi) n_hi = std::max(n_hi, fh.n[(size_t)(b0 - fh.b0 + bi)]);
  if (stride < n_hi) return "stride below the largest factored n of the range";
  for (int bi = 0; bi < count; ++bi) {
    const int n = fh.n[(size_t)(b0 - fh.b0 + bi)];
    for (int q = 0; q < nrhs; ++q) {
      const double* col = x + ((size_t)bi * nrhs + q) * (size_t)stride;
      for (int i = 0; i < n; ++i)
        if (!std::isfinite(col[i])) return "non-finite entry in the right-hand sides";
    }
  }
  *nblk_hi = (n_hi + FB - 1) / FB;
  return nullptr;
}

// Fill StepIn for pass `p` (landmarks [p*MMAX, ...)) of a validated list; `bound` is the trajectory's running
// active bound (monotone): an observed landmark and everything below it may be correlated from now on.
inline void fill_step(StepIn& s, int n_b, int& bound, double lin, double ang, int flags, const int* idx,
                      const double* range, const double* bearing, int m, int p) {
  s.lin = lin;
  s.ang = ang;
  s.flags = flags;
  const int lo = p * MMAX, cnt = std::max(0, std::min(m - lo, MMAX));
  s.m = cnt;
  for (int i = 0; i < cnt; ++i) {
    s.idx[i] = idx[lo + i];
    s.range[i] = range[lo + i];
    s.bearing[i] = bearing[lo + i];
  }
  for (int i = cnt; i < MMAX; ++i) { s.idx[i] = 0; s.range[i] = 0.0; s.bearing[i] = 0.0; }
  for (int i = 0; i < cnt; ++i) bound = std::max(bound, 3 + 2 * (s.idx[i] + 1));
  bound = std::min(bound, n_b);
  s.neff = bound;                                      // (k_solve raises it to the handle's floor, see push_floor)
  s.pad = 0;
}
// Pass p of a call plan_obs_lists accepted, into out[0, batch): the prediction in pass 0 only.  Raises the host's bound neff[b] over
// the pass's landmarks (fill_step) and sets neff_enq[b] to what the records carry.  Returns the most observations of any record.
inline int fill_step_records(HostPlan* h, bool pred, bool upd, const double* lin, const double* ang, const int* idx, const double* range,
                             const double* bearing, const int* m, int stride, int p, StepIn* out) {
  const int flags = (upd ? FLAG_UPDATE : 0) | ((pred && p == 0) ? FLAG_PREDICT : 0);
  int m_pass_hi = 0;
  for (int b = 0; b < h->batch; ++b) {
    const int mb = (upd && h->cfg.enable_measurement_model) ? m[b] : 0;
    const long off = (long)b * stride;
    fill_step(out[b], h->n[b], h->neff[b], pred ? lin[b] : 0.0, pred ? ang[b] : 0.0, flags, idx ? idx + off : nullptr,
              range ? range + off : nullptr, bearing ? bearing + off : nullptr, mb, p);
    m_pass_hi = std::max(m_pass_hi, out[b].m);
    h->neff_enq[b] = h->opt_active_bound ? h->neff[b] : h->n[b];
  }
  return m_pass_hi;
}
// Window w of arrays with `stride` detections per window, c detections, into `d`: nothing beyond them is read.
inline void fill_det_record(DetIn& d, double lin, double ang, int c, int stride, long w, const int* tag_id, const double* pose_t,
                            const double* pose_err) {
  d.lin = lin;
  d.ang = ang;
  d.count = c;
  d.pad = 0;
  for (int i = 0; i < c; ++i) {
    const long e = w * stride + i;
    d.tag_id[i] = tag_id[e];
    d.pose_err[i] = pose_err[e];
    std::copy_n(pose_t + 3 * e, 3, d.pose_t[i]);
  }
}
// The batch's windows of a call plan_det_windows accepted, into out[0, batch): count[b] detections each, nothing beyond them is read.
inline void fill_det_records(const HostPlan* h, const double* lin, const double* ang, const int* count, const int* tag_id,
                             const double* pose_t, const double* pose_err, int stride, DetIn* out) {
  for (int b = 0; b < h->batch; ++b) fill_det_record(out[b], lin[b], ang[b], count[b], stride, b, tag_id, pose_t, pose_err);
}
// The `steps` windows of a call plan_hyp_detection_stream accepted (steps = 1: plan_hyp_detections), into out[0, steps).
inline void fill_hyp_det_records(int steps, const double* lin, const double* ang, const int* count, const int* tag_id,
                                 const double* pose_t, const double* pose_err, int stride, DetIn* out) {
  for (int s = 0; s < steps; ++s) fill_det_record(out[s], lin[s], ang[s], count[s], stride, s, tag_id, pose_t, pose_err);
}

}  // namespace ekf
