// Sanitizer build of the host-side planning logic ("-fsanitize=address,undefined host build"):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DEKF_HOST_ONLY
//       -I slam-duckietown_amd/csrc -I include tests/host_plan_check.cpp -o host_plan_check
// Everything below runs the SAME source the library ships (slam-duckietown_amd/csrc/ekf_host_plan.h, ekf_device.h): the
// work queues and equal static shares of the row-slab covariance pass, the cadence / pass / step planning, the step records and
// their active bound, the validation of observation lists, the covariance's device layout, the staging layout of the read-only
// queries and the ranges of the log rings.  Enumerations (every unit /
// strip / matrix entry exactly once) plus randomised invariants; any sanitizer report or failed check ends the run with a
// non-zero status.  tests/test_cpu_host.py::test_host_planning_logic_under_the_sanitizers builds and runs it (CPU only).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "plan_check.h"

using namespace ekf;

// ---- the covariance's device layout: an injection into the allocation, row-major inside a panel ----
static void check_layout() {
  for (int ld : {64, 128, 1024, 4096, 4160, 8064, 8192, 16064, 21824}) {
    const int rows = ld > PPW ? ld : std::min(ld, 4032 + 64);
    const long alloc = p_alloc(rows, ld);
    CHECK(p_lds(ld) == std::min(ld, PPW), "ld %d", ld);
    CHECK(p_panels(ld) == (ld <= PPW ? 1 : (ld + PPW - 1) / PPW), "ld %d", ld);
    // a band of rows x every column: distinct offsets inside the allocation, consecutive along a row inside a panel
    std::set<long> seen;
    for (int i : std::set<int>{0, 1, 2, 63, rows / 2, rows - 1}) {
      for (int j = 0; j < ld; ++j) {
        const long o = p_index(ld, i, j);
        CHECK(o >= 0 && o < alloc, "ld %d (%d, %d) -> %ld of %ld", ld, i, j, o, alloc);
        CHECK(seen.insert(o).second, "ld %d (%d, %d) collides", ld, i, j);
        if (j % PPW != 0 && j > 0) CHECK(o == p_index(ld, i, j - 1) + 1, "ld %d (%d, %d) not contiguous", ld, i, j);
        CHECK((unsigned long long)p_col8(ld, (unsigned)j) == (unsigned long long)p_col(ld, j) * 8ull, "ld %d col %d", ld, j);
      }
    }
    // a 64-column strip never straddles a panel
    for (int j0 = 0; j0 + 64 <= ld; j0 += 64) CHECK(p_col(ld, j0 + 63) == p_col(ld, j0) + 63, "ld %d strip %d", ld, j0);
    // the largest byte offset fits 32 bits at the documented limit
    CHECK((unsigned long long)alloc * 8ull < (1ull << 32), "ld %d allocation", ld);
  }
  const int rows_limit = (EKF_N_MAX_LIMIT + 63) / 64 * 64;
  CHECK((unsigned long long)p_alloc(rows_limit, rows_limit) * 8ull < (1ull << 32), "limit");
  CHECK((unsigned long long)p_alloc(rows_limit + 64, rows_limit + 64) * 8ull >= (1ull << 32), "limit + 64");
}

// ---- work queues of the row-slab pass: every (trajectory, slab) once, whole or as all of its chunks ----
static void check_queues() {
  std::vector<int> buf(70000);
  for (int batch = 1; batch <= 100; batch = batch < 41 ? batch + 1 : batch + 23)
    for (int nrb : {1, 2, 5, 7, 8, 9, 15, 16, 17, 32, 126})
      for (auto [nch_in, mode] : std::vector<std::pair<int, int>>{{1, 0}, {2, 0}, {3, 0}, {2, 1}, {1, 2}, {1, 3}, {3, 3}, {8, 3}, {16, 3}}) {
        const int total = debug_pass_units(batch, nrb, nch_in, mode, buf.data(), (int)buf.size());
        CHECK(total > 0 && total <= (int)buf.size(), "batch %d nrb %d mode %d", batch, nrb, mode);
        const int nch = mode == 3 ? 2 : nch_in;
        std::map<int, int> whole, chunks;
        std::set<long> chunk_keys;
        int per_queue = 0;
        for (int g2 = 0; g2 < 8; ++g2) per_queue += rs_queue_count(g2, batch, nrb, nch_in, mode);
        CHECK(per_queue == total, "queue counts %d != %d", per_queue, total);
        for (int u = 0; u < total; ++u) {
          const int unit = buf[u];
          CHECK(unit >= 0, "negative unit");
          const int code = unit & 1023, slab = unit >> 10;
          CHECK(slab / nrb < batch, "trajectory %d of %d", slab / nrb, batch);
          if (code == 1023) ++whole[slab];
          else {
            ++chunks[slab];
            CHECK(code < nch, "chunk %d of %d", code, nch);
            CHECK(chunk_keys.insert((long)slab * 1024 + code).second, "chunk handed out twice");
          }
        }
        for (int slab = 0; slab < batch * nrb; ++slab) {
          const int w = whole.count(slab) ? whole[slab] : 0, c = chunks.count(slab) ? chunks[slab] : 0;
          CHECK((w == 1 && c == 0) || (w == 0 && c == nch), "batch %d nrb %d nch %d mode %d slab %d: %d whole, %d chunks", batch, nrb,
                nch, mode, slab, w, c);
        }
      }
}

// ---- equal static shares: every strip of every slab in exactly one piece, equal cost, any order of the shares ----
static void check_shares(std::mt19937& rng) {
  struct Case { int batch, n, wgs; };
  std::vector<Case> cases = {{1, 16003, 256}, {2, 16003, 256}, {1, 16003, 240}, {3, 12003, 256}, {7, 16003, 256}, {1, 21823, 256},
                             {3, 1403, 8},    {3, 1403, 5},    {1, 4003, 8},    {1, 16003, 255}, {4, 8003, 252},  {12, 4003, 256}};
  for (int r = 0; r < 40; ++r)
    cases.push_back({1 + (int)(rng() % 14), 3 + 2 * (int)(200 + rng() % 9000), 1 + (int)(rng() % 256)});
  for (const Case& c : cases) {
    const int pieces = pass_share_pieces();
    std::vector<int> table((size_t)c.wgs * pieces * 4, -7);
    const int longest = build_pass_shares(c.batch, c.n, c.wgs, table.data());
    if (longest == 0) continue;                        // (no table for this shape: the queue modes are used)
    CHECK(longest >= 1 && longest <= pieces, "longest %d", longest);
    for (int order = 0; order < 2; ++order) {
      if (order) order_pass_shares(c.wgs, pieces, table.data(), table.size());
      const int nrb = (c.n + RS_ROWS - 1) / RS_ROWS, s_last = (c.n - 1) >> 6;
      std::vector<int> seen((size_t)c.batch * nrb * (s_last + 1), 0);
      int cmin = 1 << 30, cmax = 0;
      for (int w = 0; w < c.wgs; ++w) {
        int cost = 0;
        bool ended = false;
        for (int k = 0; k < pieces; ++k) {
          const int* pc = &table[((size_t)w * pieces + k) * 4];
          if (pc[3] <= 0) { ended = true; continue; }
          CHECK(!ended, "a piece behind the end of share %d", w);
          CHECK(pc[0] >= 0 && pc[0] < c.batch && pc[1] >= 0 && pc[1] < nrb && pc[2] >= 0, "piece out of range");
          CHECK(pc[2] + pc[3] <= s_last - 2 * pc[1] + 1, "piece beyond its slab");
          for (int t = pc[2]; t < pc[2] + pc[3]; ++t) ++seen[((size_t)pc[0] * nrb + pc[1]) * (s_last + 1) + t];
          cost += pc[3] + 2;
        }
        cmin = std::min(cmin, cost);
        cmax = std::max(cmax, cost);
      }
      for (int b = 0; b < c.batch; ++b)
        for (int rb = 0; rb < nrb; ++rb)
          for (int t = 0; t <= s_last; ++t)
            CHECK(seen[((size_t)b * nrb + rb) * (s_last + 1) + t] == (t <= s_last - 2 * rb ? 1 : 0), "batch %d n %d wgs %d: strip (%d, %d, %d)",
                  c.batch, c.n, c.wgs, b, rb, t);
      if (c.wgs >= 5 && (long)c.batch * nrb * 4 <= (long)s_last * c.wgs) CHECK(cmax - cmin <= 4, "batch %d n %d wgs %d: costs %d..%d", c.batch, c.n, c.wgs, cmin, cmax);
    }
  }
}

// ---- planning: randomised handles ----
static HostPlan random_plan(std::mt19937& rng) {
  HostPlan h;
  h.batch = 1 + rng() % 40;
  const int N = 1 + rng() % (rng() % 4 == 0 ? 9000 : 2500);
  h.n_max = 3 + 2 * N;
  h.rows = (h.n_max + 63) / 64 * 64;
  h.ld = h.rows;
  if (h.n_max <= PPW) {
    int p2 = 64;
    while (p2 < h.n_max) p2 *= 2;
    h.ld = p2;
  }
  h.pstride = p_alloc(h.rows, h.ld);
  h.cu_count = rng() % 5 == 0 ? 64 + 8 * (int)(rng() % 25) : 256;
  h.n.resize(h.batch);
  h.neff.resize(h.batch);
  h.neff_enq.resize(h.batch);
  h.floor_host.assign(h.batch, 3);
  for (int b = 0; b < h.batch; ++b) {
    h.n[b] = 3 + 2 * (int)(rng() % (N + 1));
    h.neff[b] = std::min(h.n[b], 3 + 2 * (int)(rng() % (N + 1)));
    h.neff_enq[b] = rng() % 2 ? h.neff[b] : h.n[b];
  }
  h.sizes_dirty = rng() % 16 == 0;
  h.pending_k = 4 * (int)(rng() % 21);
  h.opt_pass_kernel = (int[]){-1, -1, -1, 0, 2}[rng() % 5];
  h.opt_pass_workgroups = rng() % 4 == 0 ? 1 + (int)(rng() % 300) : 0;
  h.opt_pass_chunk = rng() % 6 == 0 ? 1 + (int)(rng() % 80) : 0;
  h.opt_lookahead = rng() % 2;
  h.opt_streaming = (int)(rng() % 3) - 1;
  h.opt_rows_per_block = rng() % 5 == 0 ? (int)(rng() % 600) : 0;
  h.opt_flush_every = rng() % 3 == 0 ? (int)(rng() % 12) : 0;
  h.opt_rank_limit = rng() % 3 == 0 ? 2 + (int)(rng() % 79) : KTOT;
  h.opt_fused_cadence = rng() % 8 != 0;
  return h;
}

static void check_planning(std::mt19937& rng) {
  for (int it = 0; it < 4000; ++it) {
    HostPlan h = random_plan(rng);
    const PassPlan p = plan_pass(&h);
    CHECK(p.kernel == 0 || p.kernel == 2, "kernel %d", p.kernel);
    CHECK(p.nkt == (h.pending_k + 3) / 4 && p.nkt <= NKT, "nkt %d", p.nkt);
    CHECK(p.rs_workgroups >= 1 && p.rs_workgroups <= h.cu_count, "workgroups %d of %d", p.rs_workgroups, h.cu_count);
    CHECK(p.e_hi >= 3 && p.e_hi <= h.n_max && p.n_hi <= h.n_max && p.e_hi <= std::max(p.n_hi, 3), "sizes %d %d", p.e_hi, p.n_hi);
    if (h.opt_pass_kernel >= 0) CHECK(p.kernel == h.opt_pass_kernel, "forced kernel");
    if (p.beside) CHECK(p.kernel == 2 && p.long_few && p.rs_workgroups == h.cu_count - h.batch, "beside");
    const int rpb = flush_rows_per_block(&h, p.streaming, p.e_hi);
    CHECK(rpb >= 16 && rpb % 16 == 0 && rpb <= 4096 + 16, "rows per block %d", rpb);
    CHECK(flush_workgroups(p.e_hi, rpb) >= 1, "k_flush launches no workgroup");
    // the static-share table exists whenever the plan asks for it, for the size the pass covers
    if (p.kernel == 2 && p.long_few) {
      std::vector<int> table((size_t)h.cu_count * pass_share_pieces() * 4);
      const int longest = build_pass_shares(h.batch, p.e_hi, p.rs_workgroups, table.data());
      CHECK(longest >= 0 && longest <= pass_share_pieces(), "shares %d", longest);
      if (longest > 0) order_pass_shares(p.rs_workgroups, pass_share_pieces(), table.data(), table.size());
    }
    // the packed cadences of a random uploaded stream (plan_cadences): every trajectory's flat sequence of predictions and
    // landmark updates is covered exactly once, in order, within the slot and step limits
    const int steps = 1 + rng() % 120, B = h.batch;
    h.stream_steps = steps;
    h.stream_m.assign((size_t)steps * B, 0);
    h.stream_own.assign((size_t)steps * B, 3);
    h.stream_mhi.assign(steps, 0);
    const int shape = rng() % 4;                       // constant m / runs of a size / anything / mostly nothing
    int run_m = 1 + rng() % 16;
    for (int k = 0; k < steps; ++k) {
      if (rng() % 7 == 0) run_m = (int)(rng() % 17);
      for (int b = 0; b < B; ++b) {
        int m = run_m;
        if (shape == 2) m = (int)(rng() % 17);
        if (shape == 3) m = rng() % 5 == 0 ? (int)(rng() % 4) : 0;
        if (shape == 1 && b > 0) m = (int)(rng() % (run_m + 1));
        h.stream_m[(size_t)k * B + b] = (unsigned char)m;
        h.stream_own[(size_t)k * B + b] = std::min(h.n[b], 3 + 2 * (int)(rng() % ((h.n_max - 3) / 2 + 1)));
        h.stream_mhi[k] = std::max(h.stream_mhi[k], m);
      }
    }
    const int pend = h.pending_k;
    h.pending_k = 0;
    const bool dirty = h.sizes_dirty;
    h.sizes_dirty = false;
    CHECK(cadences_possible(&h) == (h.opt_fused_cadence != 0), "cadences_possible");
    const int k0 = (int)(rng() % steps), end = k0 + 1 + (int)(rng() % (steps - k0));
    RunPlan rp;
    plan_cadences(&h, k0, end, rp);
    const int slot_limit = cadence_slot_limit(&h), step_limit = cadence_step_limit(&h);
    CHECK(slot_limit >= 1 && slot_limit <= CAD_SLOTS && step_limit >= 1 && step_limit <= CAD_SLOTS, "limits %d %d", slot_limit, step_limit);
    CHECK(rp.ncad >= 1 && rp.entries.size() == (size_t)rp.ncad * B && (int)rp.slots_hi.size() == rp.ncad, "plan shape");
    long most = 0;
    for (int b = 0; b < B; ++b) {
      int t = k0, j = 0;                               // the trajectory's cursor
      long total = 0, done = 0;
      for (int c = 0; c < rp.ncad; ++c) {
        const CadPlan& e = rp.entries[(size_t)c * B + b];
        CHECK(e.t0 == t && e.j0 == j, "cadence %d of trajectory %d starts at (%d, %d), cursor (%d, %d)", c, b, e.t0, e.j0, t, j);
        CHECK(e.ns >= 0 && e.ns <= step_limit && e.nslots >= 0 && e.nslots <= slot_limit, "cadence of %d steps, %d slots", e.ns, e.nslots);
        CHECK(e.nslots <= rp.slots_hi[c], "slots_hi");
        CHECK(e.neff >= 3 && e.neff <= h.n[b], "bound %d of %d", e.neff, h.n[b]);
        if (e.ns == 0) {
          CHECK(t == end && e.nslots == 0, "an idle trajectory that is not at the end");
          continue;
        }
        CHECK(t < end, "work behind the end");
        int slots = 0;
        for (int p = 0; p < e.ns; ++p) {
          const int m = h.stream_m[(size_t)(e.t0 + p) * B + b];
          const int lo = p == 0 ? e.j0 : 0, hi = p == e.ns - 1 ? std::min(e.jend, m) : m;
          CHECK(e.t0 + p < end && lo <= hi && hi <= m, "step %d of a cadence: landmarks [%d, %d) of %d", p, lo, hi, m);
          if (p < e.ns - 1) CHECK(hi == m, "a step in the middle of a cadence is cut");
          slots += hi - lo;
        }
        CHECK(slots == e.nslots, "slots %d against %d", slots, e.nslots);
        const int m_last = h.stream_m[(size_t)(e.t0 + e.ns - 1) * B + b];
        const bool cut = e.jend < m_last;
        if (cut) CHECK(e.nslots == slot_limit, "a step is cut although %d of %d slots are free", slot_limit - e.nslots, slot_limit);
        // greedy: the cadence stops because a limit is reached or the range ends
        if (!cut && e.t0 + e.ns < end && e.ns < step_limit)
          CHECK(e.nslots == slot_limit, "cadence stops early: %d of %d slots, %d of %d steps", e.nslots, slot_limit, e.ns, step_limit);
        done += e.ns - (cut ? 1 : 0);
        t = e.t0 + e.ns - (cut ? 1 : 0);
        j = cut ? e.jend : 0;
        total += slots;
      }
      CHECK(t == end && j == 0, "trajectory %d ends at (%d, %d), not at %d", b, t, j, end);
      long want = 0;
      for (int k = k0; k < end; ++k) want += h.stream_m[(size_t)k * B + b];
      CHECK(total == want, "landmark updates %ld of %ld", total, want);
      most = std::max(most, want);
    }
    // as many cadences as the busiest trajectory needs, when only the slots limit them
    if (step_limit == CAD_SLOTS && most > 0) {
      long steps_bound = (end - k0 + CAD_SLOTS - 1) / CAD_SLOTS;
      CHECK(rp.ncad <= std::max((most + slot_limit - 1) / slot_limit, 1L) + steps_bound, "%d cadences for %ld updates", rp.ncad, most);
    }
    h.sizes_dirty = dirty;
    h.pending_k = pend;
  }
}

// ---- what the launchers are handed: the pass's hand-out, the per-step form, the fused cadence's follow-up, the small path ----
// (every unit of a row-slab plan's work queues names a (trajectory, slab) of the batch; each one comes whole or as all its chunks)
static void check_handout(int batch, int nrb, int nch, int mode, int grid, std::vector<int>& buf) {
  const int total = debug_pass_units(batch, nrb, nch, mode, nullptr, 0);
  buf.assign((size_t)total, -1);
  CHECK(debug_pass_units(batch, nrb, nch, mode, buf.data(), total) == total, "unit count");
  CHECK(grid >= 1 && grid <= total, "grid %d for %d units (batch %d nrb %d nch %d mode %d)", grid, total, batch, nrb, nch, mode);
  const int chunks_per_slab = mode == 3 ? 2 : nch;
  std::vector<int> whole((size_t)batch * nrb, 0), parts((size_t)batch * nrb, 0);
  std::set<long> keys;
  for (int u = 0; u < total; ++u) {
    const int code = buf[u] & 1023, slab = buf[u] >> 10;
    CHECK(buf[u] >= 0 && slab < batch * nrb, "unit %d of mode %d", buf[u], mode);
    if (code == 1023) ++whole[slab];
    else {
      CHECK(code < chunks_per_slab && keys.insert((long)slab * 1024 + code).second, "chunk %d of slab %d", code, slab);
      ++parts[slab];
    }
  }
  for (int slab = 0; slab < batch * nrb; ++slab)
    CHECK((whole[slab] == 1 && parts[slab] == 0) || (whole[slab] == 0 && parts[slab] == chunks_per_slab),
          "batch %d nrb %d nch %d mode %d: slab %d %d whole, %d chunks", batch, nrb, nch, mode, slab, whole[slab], parts[slab]);
}

static void check_launch_plans(std::mt19937& rng) {
  std::vector<int> buf;
  for (int it = 0; it < 6000; ++it) {
    HostPlan h = random_plan(rng);
    if (rng() % 8 == 0) {                              // (banks of small filters)
      h.batch = 1 + rng() % 1200;
      h.n.assign(h.batch, h.n_max);
      h.neff.assign(h.batch, h.n_max);
      h.neff_enq.assign(h.batch, h.n_max);
      h.floor_host.assign(h.batch, 3);
    }
    h.pending_k = rng() % 3 == 0 ? 0 : 2 * (int)(rng() % 41);
    h.pending_steps = (int)(rng() % 41);
    h.opt_fused_step = (int)(rng() % 3);
    h.opt_small_state = rng() % 4 != 0;
    h.opt_chain = rng() % 4 != 0;
    h.opt_w_from_v = rng() % 4 != 0;
    h.opt_panel_shape = rng() % 3 == 0 ? (int)(rng() % 4) : 0;
    h.opt_panel_tform = rng() % 4 != 0;
    h.opt_col_gather = rng() % 4 != 0;
    h.chain_run = rng() % 2;
    // the covariance pass, as the handle stands and as asked about (any pending ranks, every index active)
    for (int q = 0; q < 2; ++q) {
      const PassPlan p = q == 0 ? plan_pass(&h) : plan_pass(&h, KTOT, true);
      if (q == 1) CHECK(p.nkt == NKT && p.e_hi >= (h.sizes_dirty ? h.n_max : p.n_hi), "hypothetical pass %d %d", p.nkt, p.e_hi);
      if (p.kernel == 0) CHECK(p.rows_per_block == flush_rows_per_block(&h, p.streaming, p.e_hi), "rows per block");
      if (p.kernel == 2 && (long)h.batch * ((p.e_hi + 127) / 128) * ((p.e_hi + 63) / 64) <= 400000)
        check_handout(h.batch, (p.e_hi + RS_ROWS - 1) / RS_ROWS, p.rs_nch, p.rs_mode, p.rs_grid, buf);
    }
    // the per-step update
    const int n_hi = h.sizes_dirty ? h.n_max : *std::max_element(h.n.begin(), h.n.end());
    for (int m_hi : {0, 1, 3, 5, 8, 9, 16}) {
      const StepPlan s = plan_step(&h, m_hi, n_hi);
      CHECK(s.mcap >= m_hi && s.mcap <= 16, "mcap %d for %d", s.mcap, m_hi);
      CHECK((s.form == STEP_PREDICT) == (m_hi == 0 && h.pending_k == 0), "prediction-only form");
      if (s.form == STEP_SPLIT || s.form == STEP_SPLIT_TP) CHECK(h.opt_fused_step != 0, "single launch without fused_step");
      if (s.form == STEP_SPLIT_TP) CHECK(s.mcap <= 8 && !s.panels_latency, "throughput form with mcap %d", s.mcap);
      if (s.form == STEP_SPLIT) CHECK(step_is_split(h.batch, n_hi, h.cu_count), "split form");
      CHECK(s.flush_before == (s.form != STEP_PREDICT && ((h.pending_k + 2 * s.mcap + 3) & ~3) > KTOT), "flush before");
      // behind the step (its ranks appended): no pending count beyond the rank slots survives
      HostPlan a = h;
      a.pending_k = (s.flush_before ? 0 : h.pending_k) + 2 * m_hi;
      a.pending_steps = (s.flush_before ? 0 : h.pending_steps) + 1;
      if (a.pending_k + 2 > KTOT) CHECK(pass_due_after_step(&a, m_hi), "ranks left pending beyond the slots");
    }
    // the small-state path: the kernel's tiles cover the state, its forms stay within their size limits
    if (small_path(&h)) CHECK(h.pending_k == 0 && h.n_max <= small_state_limit(h.batch) && h.n_max <= SMALL_N_MAX_BANK, "small path");
    const int sf = plan_small(&h, n_hi), sn = std::min(n_hi, SMALL_N_MAX_BANK);
    const int tiles[] = {3, 3, 5, 7, 9};
    CHECK(sf >= SMALL_OCC_3 && sf <= SMALL_9 && 16 * tiles[sf] >= sn, "small form %d for n %d", sf, sn);
    if (sf == SMALL_OCC_3) CHECK(h.batch > 3 * h.cu_count && sn <= 48, "many small filters");
    if (sf == SMALL_3 || sf == SMALL_5) CHECK(sn <= (sf == SMALL_3 ? 48 : 80), "small form %d for n %d", sf, sn);
    if (sf == SMALL_TWO_7) CHECK(sn > 80 && sn <= 112, "two-per-CU form for n %d", sn);
    // chained runs and the fused cadence's follow-up
    const int gw = chain_gather_workgroups(h.batch, h.cu_count);
    CHECK(gw >= 1 && gw <= CH_GW, "gather workgroups %d", gw);
    RunPlan rp;
    rp.ncad = 1 + (int)(rng() % 4);
    for (int c = 0; c < rp.ncad; ++c) {
      rp.slots_hi.push_back(rng() % 5 == 0 ? 0 : 1 + (int)(rng() % CAD_SLOTS));
      rp.steps_hi.push_back((int)(rng() % (CAD_SLOTS + 1)));
    }
    if (plan_chain_run(&h, rp.ncad))
      CHECK(h.batch <= 40 && rp.ncad >= 2 && h.opt_chain && h.opt_lookahead, "chained run of %d cadences, batch %d", rp.ncad, h.batch);
    if (h.sizes_dirty) continue;                       // (cadences run on sizes read back)
    for (int c = 0; c < rp.ncad; ++c)
      for (int pre = 0; pre < 2; ++pre) {
        const CadStepPlan p = plan_cadence_step(&h, rp, c, n_hi, pre);
        const bool latency = panels_cad_latency_regime(h.batch, n_hi);
        CHECK(p.panel >= PANEL_TF && p.panel <= PANEL_FOUR, "panel form %d", p.panel);
        if (p.gather_cols) CHECK(!pre && rp.slots_hi[c] > 0 && p.col_wgs > 0 && h.opt_col_gather, "column gather");
        if (p.beside) CHECK(p.due && c + 1 < rp.ncad && h.opt_lookahead, "beside");
        if (p.chain_next) CHECK(p.beside && h.chain_run && p.due, "chain_next");
        if (p.w_from_v)
          CHECK(p.due && !p.beside && h.pending_k == 0 && plan_pass(&h, 2 * rp.slots_hi[c]).kernel == 2 &&
                (p.panel == PANEL_ONE || p.panel == PANEL_FOUR), "w_from_v");
        if (p.panel == PANEL_TF) CHECK(p.chain_next && !p.gather_cols && latency && h.opt_panel_tform, "triangular-solve form");
        else if (h.opt_panel_shape > 0) CHECK(p.panel == PANEL_KS + h.opt_panel_shape - 1, "panel_shape %d: form %d", h.opt_panel_shape, p.panel);
        else CHECK((p.panel == PANEL_KS) == latency, "panel form %d", p.panel);
      }
  }
}

// ---- a run's launch order (plan_cadence_launches): whole runs walked cadence by cadence on a model of the two in-order queues
// and the four device-scope counters of ekf_cadence.hip, carrying CadRun and the pending counts as enqueue_cadence does ----
struct OrderModel {
  long seq = 0;                                        // the global enqueue sequence, across cadences, pieces and both streams
  std::set<unsigned> solve_done, pass_done, solve_started, gathers_done;   // values SYNC_SOLVE / _PASS / _START / _GATHER will reach: their producers are enqueued
  bool mark_outstanding = false;                       // a mark is on the second stream and the handle's has not waited for it
  int aux_open = 0;                                    // launches on the second stream no join covers yet
  long pre_serial[2] = {-1, -1};                       // whose inputs a CadPre copy holds ...
  int pre_piece[2] = {-1, -1}, piece = 0;              // ... and the piece that formed them
  int ahead_set = -1;                                  // the buffer set the solve enqueued ahead writes (-1: none ahead)
  long chained = 0, lookahead = 0, serial = 0;         // transitions walked, by order
};
enum { ORDER_SERIAL, ORDER_LOOKAHEAD, ORDER_CHAINED };

// One piece of a run (ekf_stream_run: plan_chain_run, the cadences, join_aux).  `want`: the order every cadence but the last
// must take (-1: any); the last is serial.
static void walk_piece(HostPlan& h, const RunPlan& rp, int n_hi, OrderModel& M, int want) {
  h.chain_run = plan_chain_run(&h, rp.ncad);          // (ekf_api.hip: prepare_piece)
  const int gw = h.chain_gw = chain_gather_workgroups(h.batch, h.cu_count);
  bool presolved = false;
  for (int c = 0; c < rp.ncad; ++c) {
    const HostPlan before = h;
    const CadStepPlan cp = plan_cadence_step(&before, rp, c, n_hi, presolved);
    const CadLaunches L = plan_cadence_launches(&h, rp, c, n_hi, presolved);
    const CadRun &r0 = before.run, &r1 = h.run;
    const long serial = r0.cad_serial;
    const int ranks = 2 * rp.slots_hi[c], pend_after = before.pending_k + ranks;
    CHECK(L.n >= 1 && L.n <= CAD_OPS_MAX, "%d ops", L.n);
    const CadOp *chain = nullptr, *ahead = nullptr, *own = nullptr, *panel = nullptr, *pass = nullptr, *gate = nullptr;
    bool fork = false, join = false, committed = false;
    const int solved_into = presolved ? M.ahead_set : -1;   // the set the previous cadence's list had this one's solve write
    std::vector<int> on[2];                            // the kinds per stream, in order (the logs and the leading join apart)
    for (int i = 0; i < L.n; ++i) {
      const CadOp& op = L.op[i];
      ++M.seq;
      CHECK(op.stream == ON_MAIN || op.stream == ON_AUX, "stream %d", op.stream);
      CHECK(op.which == CAD_THIS || op.which == CAD_NEXT, "which %d", op.which);
      if (op.no_way_back) CHECK(op.kind == OP_SOLVE && op.which == CAD_NEXT && !committed, "no-way-back mark on op %d", op.kind);
      committed = committed || op.no_way_back;
      if (op.kind != OP_LOG && op.kind != OP_JOIN_AUX) on[op.stream].push_back(op.kind);
      if (op.stream == ON_AUX && op.kind != OP_JOIN) M.aux_open += 1;
      switch (op.kind) {
        case OP_JOIN_AUX:
          CHECK(i == 0 && op.stream == ON_MAIN && r0.aux_pass && M.mark_outstanding, "JOIN_AUX at %d", i);
          M.mark_outstanding = false, M.aux_open = 0;
          break;
        case OP_SOLVE:
          CHECK(op.stream == ON_MAIN && op.cls == 1, "solve on %d class %d", op.stream, op.cls);
          if (op.which == CAD_THIS) {
            own = &op;
            CHECK(!presolved && !M.mark_outstanding && !chain && !panel, "a cadence's own solve");   // (behind everything on the second stream)
            CHECK(!op.sync && op.gparts == 0 && op.pre_in < 0 && op.chain == before.chain_run, "own solve's arguments");
          } else {
            ahead = &op;
            M.ahead_set = r0.cpar ^ CAD_NEXT;
            CHECK(c + 1 < rp.ncad && op.gparts >= 1 && !op.colbuf && op.col_wgs == 0, "solve ahead");
            // chained: block and mean are the chain launch's, already in this queue.  The solve itself waits on no counter
            // (ekf_solve_cad_body.inc): with start_sigma it only ANNOUNCES that it has been placed (SYNC_START), for its panel
            if (op.sync) {
              CHECK(chain && op.sigma == chain->sigma && op.gparts == 1 && op.chain && op.pre_in == chain->pre_in, "chained solve");
              M.solve_started.insert(op.sigma);
            } else {
              CHECK(fork && op.sigma == 0 && op.pre_in < 0 && op.chain == before.chain_run, "look-ahead solve");
            }
          }
          break;
        case OP_LOG: CHECK(op.stream == ON_MAIN && i > 0 && L.op[i - 1].kind == OP_SOLVE && L.op[i - 1].which == op.which, "log"); break;
        case OP_CHAIN:
          chain = &op;
          CHECK(op.stream == ON_MAIN && op.which == CAD_NEXT && op.cls == 2, "chain");
          CHECK(op.sigma == r0.sigma + 1u && op.target == r0.gather_count + (unsigned)(h.batch * gw) && op.gw == gw, "chain counters");
          CHECK(op.wait_pass == M.mark_outstanding, "wait_pass %d, a mark outstanding %d", op.wait_pass, M.mark_outstanding);
          if (op.wait_pass) CHECK(M.pass_done.count(op.sigma - 1u), "the chain's gathers wait for a mark that is not enqueued");
          if (op.pre_in >= 0)
            CHECK(M.pre_serial[op.pre_in] == serial + 1 && M.pre_piece[op.pre_in] == M.piece, "pre_in: copy %d holds %ld of piece %d", op.pre_in,
                  M.pre_serial[op.pre_in], M.pre_piece[op.pre_in]);
          else
            for (int q = 0; q < 2; ++q) CHECK(!(M.pre_serial[q] == serial + 1 && M.pre_piece[q] == M.piece), "inputs formed ahead are not used");
          CHECK((op.pre_out >= 0) == (c + 2 < rp.ncad) && op.plan2 == (op.pre_out >= 0) && (op.pre_out < 0 || op.pre_out != op.pre_in), "pre_out");
          if (op.pre_out >= 0) M.pre_serial[op.pre_out] = serial + 2, M.pre_piece[op.pre_out] = M.piece;
          M.solve_done.insert(op.sigma);               // (its start announces this cadence's solve, in front of it on the stream)
          M.gathers_done.insert(op.target);
          break;
        case OP_GATE:
          gate = &op;
          CHECK(op.stream == ON_AUX && M.solve_done.count(op.sigma), "the gate waits for a chain launch that is not enqueued");
          break;
        case OP_PANEL:
          panel = &op;
          CHECK(op.which == CAD_THIS && op.cls == 3 && op.nrp == ((ranks + 3) & ~3) && op.ranks == ranks && op.form == cp.panel, "panel");
          CHECK(op.skipw == cp.w_from_v && op.colbuf == cp.gather_cols && op.keep_prow3 == before.chain_run, "panel flags");
          CHECK(presolved ? solved_into == r0.cpar : solved_into < 0, "the panel reads set %d, the solve ahead wrote %d", r0.cpar, solved_into);
          if (op.sync) {
            CHECK(op.stream == ON_AUX && chain && gate && ahead, "chained panel");
            CHECK(op.target == chain->target && op.sigma == chain->sigma, "tail_target %u, gather_target %u", op.target, chain->target);
            CHECK(M.gathers_done.count(op.target) && M.solve_started.count(op.sigma), "the panel waits for launches that are not enqueued");
          } else {
            CHECK(op.stream == ON_MAIN && !chain && !M.mark_outstanding, "panel on the handle's stream");
          }
          h.pending_k += op.ranks, h.pending_steps = op.steps_after;
          CHECK(h.pending_steps == (pend_after == 0 ? 0 : before.pending_steps + rp.steps_hi[c]), "pending steps");
          break;
        case OP_PASS:
          pass = &op;
          CHECK(panel && h.pending_k > 0 && op.cls == 0 && op.wv == (cp.w_from_v && op.stream == ON_MAIN), "pass");
          h.pending_k = 0, h.pending_steps = 0;
          break;
        case OP_MARK:
          CHECK(op.stream == ON_AUX && pass && chain && op.sigma == chain->sigma && i == L.n - 1, "mark");
          M.pass_done.insert(op.sigma);
          M.mark_outstanding = true;
          break;
        case OP_GATHER:
          CHECK(op.stream == ON_MAIN && op.which == CAD_NEXT && op.cls == 2 && panel && op.kb == ((h.pending_k + 3) & ~3) && op.kb > 0, "gather");
          break;
        case OP_FORK:
          CHECK(op.stream == ON_MAIN && !fork && M.aux_open == 0, "fork");
          fork = true;
          break;
        case OP_JOIN:
          CHECK(op.stream == ON_AUX && fork && !join && i == L.n - 1, "join");
          join = true, M.aux_open = 0;
          break;
        default: CHECK(false, "op kind %d", op.kind);
      }
    }
    CHECK(fork == join, "a fork without its join in the same cadence");
    CHECK((own != nullptr) == !presolved, "presolved %d, own solve %d", presolved, own != nullptr);
    if (own) CHECK(own->colbuf == cp.gather_cols && own->col_wgs == cp.col_wgs, "column gather");
    // per-stream order, by the order the list takes
    const int order = chain ? ORDER_CHAINED : fork ? ORDER_LOOKAHEAD : ORDER_SERIAL;
    std::vector<int> main_want, aux_want;
    if (own) main_want.push_back(OP_SOLVE);
    if (order == ORDER_CHAINED) {
      main_want.insert(main_want.end(), {OP_CHAIN, OP_SOLVE});
      aux_want = {OP_GATE, OP_PANEL, OP_PASS, OP_MARK};
      M.chained += 1;
    } else if (order == ORDER_LOOKAHEAD) {
      main_want.insert(main_want.end(), {OP_PANEL, OP_GATHER, OP_FORK, OP_SOLVE});
      aux_want = {OP_PASS, OP_JOIN};
      M.lookahead += 1;
    } else {
      main_want.push_back(OP_PANEL);
      if (cp.due && pend_after > 0) main_want.push_back(OP_PASS);
      M.serial += 1;
    }
    CHECK(on[ON_MAIN] == main_want && on[ON_AUX] == aux_want, "cadence %d of %d: order %d, %zu + %zu ops", c, rp.ncad, order, on[ON_MAIN].size(),
          on[ON_AUX].size());
    if (want >= 0) CHECK(order == (c + 1 < rp.ncad ? want : ORDER_SERIAL), "cadence %d of %d takes order %d, not %d", c, rp.ncad, order, want);
    // agreement with plan_cadence_step, the counters and the statistics
    CHECK((pass != nullptr) == (cp.due && pend_after > 0) && (order != ORDER_SERIAL) == cp.beside && (order == ORDER_CHAINED) == cp.chain_next, "flags");
    CHECK(L.next_presolved == (order != ORDER_SERIAL) && (ahead != nullptr) == L.next_presolved, "next_presolved");
    CHECK(r1.cad_serial == serial + 1 && r1.cpar == (r0.cpar ^ 1) && h.chain_run == before.chain_run, "serial and parity");
    CHECK(r1.sigma == r0.sigma + (order == ORDER_CHAINED ? 1u : 0u), "sigma");
    CHECK(r1.gather_count == r0.gather_count + (order == ORDER_CHAINED ? (unsigned)(h.batch * gw) : 0u), "gather_count");
    CHECK(r1.aux_pass == M.mark_outstanding, "aux_pass %d, a mark outstanding %d", r1.aux_pass, M.mark_outstanding);
    for (int q = 0; q < 2; ++q)
      if (M.pre_piece[q] == M.piece) CHECK(r1.pre_serial[q] == M.pre_serial[q], "pre_serial[%d]", q);
    CHECK(r1.cadences == r0.cadences + 1 && r1.cadence_traj_steps == r0.cadence_traj_steps + rp.steps_sum[c], "cadence statistics");
    CHECK(r1.lookaheads == r0.lookaheads + (order != ORDER_SERIAL) && r1.chained == r0.chained + (order == ORDER_CHAINED), "look-ahead statistics");
    CHECK(r1.w_from_v_passes == r0.w_from_v_passes + (order == ORDER_SERIAL && pass && cp.w_from_v), "w_from_v statistics");
    if (order != ORDER_CHAINED) CHECK(M.aux_open == 0, "launches left on the second stream behind a cadence that is not chained");
    if (!L.next_presolved) M.ahead_set = -1;
    presolved = L.next_presolved;
  }
  CHECK(!presolved, "a solve enqueued ahead of a run's end");
  if (h.run.aux_pass) {                                // ekf_stream_run's join_aux behind the last cadence
    ++M.seq;
    h.run.aux_pass = false, M.mark_outstanding = false, M.aux_open = 0;
  }
  CHECK(M.aux_open == 0 && !M.mark_outstanding, "launches outstanding on the second stream behind a run");
  M.piece += 1;
}

static RunPlan run_of(const std::vector<int>& slots, int steps_each, int batch) {
  RunPlan rp;
  rp.ncad = (int)slots.size();
  rp.slots_hi = slots;
  rp.steps_hi.assign(slots.size(), steps_each);
  rp.steps_sum.assign(slots.size(), (long)steps_each * batch);
  return rp;
}

static void check_cadence_orders(std::mt19937& rng) {
  OrderModel total;
  // the random handles of check_launch_plans, runs of 1 .. 6 cadences, a second piece on the same state
  for (int it = 0; it < 6000; ++it) {
    HostPlan h = random_plan(rng);
    h.sizes_dirty = false;                             // (cadences run on sizes read back, with nothing pending)
    h.pending_k = h.pending_steps = 0;
    h.opt_chain = rng() % 4 != 0;
    h.opt_w_from_v = rng() % 4 != 0;
    h.opt_panel_shape = rng() % 3 == 0 ? (int)(rng() % 4) : 0;
    h.opt_panel_tform = rng() % 4 != 0;
    h.opt_col_gather = rng() % 4 != 0;
    if (rng() % 2) h.neff = h.neff_enq = h.n;          // (every index active: where a pass is long enough for a solve beside it)
    const int n_hi = *std::max_element(h.n.begin(), h.n.end());
    OrderModel M;
    for (int piece = 0; piece < 2; ++piece) {
      std::vector<int> slots(1 + rng() % 6);
      for (int& s : slots) s = rng() % 5 == 0 ? 0 : rng() % 3 == 0 ? CAD_SLOTS : 1 + (int)(rng() % CAD_SLOTS);
      walk_piece(h, run_of(slots, (int)(rng() % (CAD_SLOTS + 1)), h.batch), n_hi, M, -1);
      h.pending_k = h.pending_steps = 0;               // (between two pieces what the last cadence left pending is applied)
    }
    total.chained += M.chained, total.lookahead += M.lookahead, total.serial += M.serial;
  }
  CHECK(total.chained > 0 && total.lookahead > 0, "the random draws walked %ld chained and %ld look-ahead transitions", total.chained, total.lookahead);
  std::printf("cadence orders walked by the random draws alone: %ld chained, %ld look-ahead, %ld serial transitions\n", total.chained,
              total.lookahead, total.serial);
  // fixed cases: 256 CUs, every index active, nothing pending, runs of 1, 2 and 3 full cadences (the last one's pass is due: its
  // slots are used up), two pieces each
  struct Fixed { int batch, N, lookahead, chain, want; };
  const Fixed fixed[] = {{1, 100, 1, 1, ORDER_CHAINED}, {2, 100, 1, 1, ORDER_CHAINED}, {40, 100, 1, 1, ORDER_CHAINED},
                         {1, 1250, 1, 0, ORDER_LOOKAHEAD},
                         {1, 100, 0, 1, ORDER_SERIAL},  {1, 100, 1, 0, ORDER_SERIAL}, {41, 100, 1, 1, ORDER_SERIAL}, {32, 2000, 1, 1, ORDER_SERIAL}};
  for (const Fixed& f : fixed)
    for (int ncad = 1; ncad <= 3; ++ncad) {
      HostPlan h = bank(3 + 2 * f.N, std::vector<int>(f.batch, 3 + 2 * f.N));
      h.cu_count = 256;
      h.floor_host.assign(f.batch, 3);
      h.opt_lookahead = f.lookahead, h.opt_chain = f.chain;
      OrderModel M;
      for (int piece = 0; piece < 2; ++piece) {
        const RunPlan rp = run_of(std::vector<int>(ncad, CAD_SLOTS), 5, f.batch);
        walk_piece(h, rp, h.n_max, M, f.want);
        CHECK(h.pending_k == 0, "a run whose last cadence uses its slots up leaves %d ranks pending", h.pending_k);
        if (f.batch == 32 && f.N == 2000) {
          const CadStepPlan cp = plan_cadence_step(&h, rp, 0, h.n_max, false);
          CHECK(cp.w_from_v && cp.panel == PANEL_FOUR && h.run.w_from_v_passes == (long)ncad * (piece + 1), "the headline bank's form");
        }
      }
      total.chained += M.chained, total.lookahead += M.lookahead, total.serial += M.serial;
    }
  {                                                    // a cadence that observes nothing with nothing pending: the panel launch applies the noise
    HostPlan h = bank(203, std::vector<int>(1, 203));
    h.cu_count = 256;
    h.floor_host.assign(1, 3);
    OrderModel M;
    walk_piece(h, run_of({0, CAD_SLOTS, 0, 7}, 5, 1), h.n_max, M, -1);
    CHECK(h.pending_k == 14 && M.chained + M.lookahead + M.serial == 4, "a run with empty cadences");
    total.chained += M.chained, total.lookahead += M.lookahead, total.serial += M.serial;
  }
  CHECK(total.chained > 0 && total.lookahead > 0 && total.serial > 0, "an order was never walked");
  std::printf("cadence orders walked: %ld chained, %ld look-ahead, %ld serial transitions\n", total.chained, total.lookahead, total.serial);
}

static void check_step_records(std::mt19937& rng) {
  for (int it = 0; it < 3000; ++it) {
    HostPlan h;
    h.batch = 1;
    const int n_lm = 1 + rng() % 300;
    h.n = {3 + 2 * n_lm};
    const int m = rng() % 40;
    std::vector<int> idx(m);
    std::vector<double> r(m), bq(m);
    bool dup = false, oob = false;
    std::set<int> used;
    for (int i = 0; i < m; ++i) {
      idx[i] = (int)(rng() % (n_lm + (rng() % 9 == 0 ? 3 : 0))) - (rng() % 50 == 0 ? 1 : 0);
      if (idx[i] < 0 || idx[i] >= n_lm) oob = true;
      else if (!used.insert(idx[i]).second) dup = true;
      r[i] = 0.1 * i;
      bq[i] = -0.01 * i;
    }
    std::vector<unsigned char> seen;
    const char* why = validate_obs(&h, 0, idx.data(), m, seen);
    CHECK((why != nullptr) == (dup || oob), "validate_obs: %s with dup=%d oob=%d", why ? why : "accepted", dup, oob);
    if (why) continue;
    int bound = 3 + 2 * (int)(rng() % (n_lm + 1)), prev = bound;
    int taken = 0;
    for (int p = 0; p < std::max(1, (m + MMAX - 1) / MMAX); ++p) {
      StepIn s;
      std::memset(&s, 0xAB, sizeof s);
      fill_step(s, h.n[0], bound, 0.004, 0.02, FLAG_PREDICT | FLAG_UPDATE, idx.data(), r.data(), bq.data(), m, p);
      CHECK(s.m == std::max(0, std::min(m - p * MMAX, MMAX)), "pass %d takes %d of %d", p, s.m, m);
      for (int i = 0; i < MMAX; ++i) {
        if (i < s.m) CHECK(s.idx[i] == idx[p * MMAX + i] && s.range[i] == r[p * MMAX + i] && s.bearing[i] == bq[p * MMAX + i], "record entry %d", i);
        else CHECK(s.idx[i] == 0 && s.range[i] == 0.0 && s.bearing[i] == 0.0, "padding entry %d", i);
      }
      CHECK(bound >= prev && bound <= h.n[0] && s.neff == bound, "bound %d -> %d (n %d)", prev, bound, h.n[0]);
      for (int i = 0; i < s.m; ++i) CHECK(bound >= std::min(h.n[0], 3 + 2 * (s.idx[i] + 1)), "observed landmark beyond the bound");
      prev = bound;
      taken += s.m;
    }
    CHECK(taken == m, "passes took %d of %d", taken, m);
  }
}

// The shared planner of the observation lists (plan_obs_lists: ekf_step / _update / _predict, ekf_localize_step / _update,
// ekf_stream_upload per step) in both modes, and the record fill of a planned call (fill_step_records).  Every call is generated
// with its faults known -- a NULL it needs, a count outside [0, stride], an index outside the map, a duplicate -- and the planner
// refuses exactly the calls that have one it reads; arrays have exactly the stated size.
static void check_obs_planner(std::mt19937& rng) {
  int refused = 0, accepted = 0, empty_null = 0, update_only = 0;
  for (int it = 0; it < 6000; ++it) {
    const int batch = rng() % 2 ? 1 : 3;
    const int strides[] = {0, 1, 16, 17, 33}, stride = strides[rng() % 5];
    std::vector<int> n;
    for (int b = 0; b < batch; ++b) n.push_back(3 + 2 * (b == 0 ? 33 + (int)(rng() % 20) : b == 1 ? 1 + (int)(rng() % 5) : 17));
    std::vector<int> neff;
    for (int b = 0; b < batch; ++b) neff.push_back(3 + 2 * (int)(rng() % ((n[(size_t)b] - 3) / 2 + 1)));
    HostPlan h = bank(3 + 2 * 60, n, neff);
    h.cfg.enable_measurement_model = rng() % 4 != 0;
    h.opt_active_bound = rng() % 5 != 0;
    const bool meas = h.cfg.enable_measurement_model != 0, unique = rng() % 2 == 0;
    const bool pred = rng() % 3 != 0, upd = !pred || rng() % 3 != 0;
    // the call: distinct indices inside each map, in random order
    std::vector<double> lin((size_t)batch, 0.004), ang((size_t)batch, 0.02), range((size_t)batch * stride), bearing((size_t)batch * stride);
    std::vector<int> idx((size_t)batch * stride, 0), m((size_t)batch, 0);
    const bool nothing = rng() % 6 == 0;
    for (int b = 0; b < batch; ++b) {
      const int nl = (n[(size_t)b] - 3) / 2;
      m[(size_t)b] = nothing ? 0 : (int)(rng() % (std::min(stride, nl) + 1));
      std::vector<int> perm((size_t)nl);
      for (int i = 0; i < nl; ++i) perm[(size_t)i] = i;
      std::shuffle(perm.begin(), perm.end(), rng);
      for (int i = 0; i < m[(size_t)b]; ++i) {
        idx[(size_t)b * stride + i] = perm[(size_t)i];
        range[(size_t)b * stride + i] = 1.0 + 0.01 * i + b;
        bearing[(size_t)b * stride + i] = 0.1 - 0.001 * i;
      }
    }
    // the faults
    const bool null_motion = rng() % 8 == 0, null_m = rng() % 12 == 0, null_obs = rng() % 8 == 0;
    bool bad_count = false, outside = false, dup = false;
    const int fb = (int)(rng() % batch);
    if (rng() % 8 == 0) {
      m[(size_t)fb] = rng() % 2 ? stride + 1 : -1;
      bad_count = true;
    }
    int m_hi = 0;
    for (int b = 0; b < batch; ++b) m_hi = std::max(m_hi, m[(size_t)b]);
    if (!bad_count && m[(size_t)fb] > 0 && rng() % 6 == 0) {
      idx[(size_t)fb * stride + rng() % m[(size_t)fb]] = rng() % 2 ? (n[(size_t)fb] - 3) / 2 + (int)(rng() % 2) : -1;
      outside = true;
    }
    if (!bad_count && !outside && m[(size_t)fb] > 1 && rng() % 6 == 0) {
      const int i = 1 + (int)(rng() % (m[(size_t)fb] - 1));
      idx[(size_t)fb * stride + i] = idx[(size_t)fb * stride + rng() % i];
      dup = true;
    }
    const bool lists_read = upd && meas && !null_m && !bad_count && m_hi > 0;
    const bool want_refused = (pred && null_motion) || (upd && null_m) || (upd && meas && !null_m && bad_count) ||
                              (lists_read && (null_obs || outside || (unique && dup)));
    const unsigned gone_motion = null_motion ? 1 + rng() % 3 : 0, gone_obs = null_obs ? 1 + rng() % 7 : 0;   // (bit sets: which are NULL)
    const double *plin = gone_motion & 1 ? nullptr : lin.data(), *pang = gone_motion & 2 ? nullptr : ang.data();
    const int* pidx = gone_obs & 1 ? nullptr : idx.data();
    const double *prange = gone_obs & 2 ? nullptr : range.data(), *pbearing = gone_obs & 4 ? nullptr : bearing.data();
    ObsPlan op;
    const char* why = plan_obs_lists(&h, pred, upd, unique, plin, pang, pidx, prange, pbearing, null_m ? nullptr : m.data(), stride, op);
    CHECK((why != nullptr) == want_refused,
          "trial %d: %s (pred %d upd %d meas %d unique %d; NULL motion %d m %d lists %d; bad count %d outside %d dup %d; m_hi %d)", it,
          why ? why : "accepted", pred, upd, meas, unique, null_motion, null_m, null_obs, bad_count, outside, dup, m_hi);
    if (why) {
      ++refused;
      continue;
    }
    ++accepted;
    const int want_hi = upd && meas ? m_hi : 0;        // (a direct count: nothing is observed with the model off or without an update)
    CHECK(op.m_hi == want_hi && op.passes == std::max(1, (want_hi + MMAX - 1) / MMAX), "trial %d: m_hi %d passes %d for %d", it, op.m_hi,
          op.passes, want_hi);
    empty_null += want_hi == 0 && null_obs;
    update_only += !pred && null_motion;
    LocPlan lp;                                          // (what SLAM takes localisation takes, with the same plan)
    CHECK(plan_localize(&h, pred, upd, plin, pang, pidx, prange, pbearing, null_m ? nullptr : m.data(), stride, lp) == nullptr &&
              lp.m_hi == op.m_hi && lp.passes == op.passes, "trial %d: plan_localize differs", it);
    // ---- the records of the planned call: fill_step_records against a plain loop over fill_step ----
    HostPlan g = h, ref = h;
    std::vector<int> got_idx[3];
    for (int p = 0; p < op.passes; ++p) {
      std::vector<StepIn> out((size_t)batch), want((size_t)batch);
      std::memset(out.data(), 0xAB, sizeof(StepIn) * out.size());
      std::memset(want.data(), 0xAB, sizeof(StepIn) * want.size());
      const std::vector<int> before = g.neff;
      const int pass_hi = fill_step_records(&g, pred, upd, plin, pang, pidx, prange, pbearing, null_m ? nullptr : m.data(), stride, p, out.data());
      int want_pass_hi = 0;
      for (int b = 0; b < batch; ++b) {
        const long off = (long)b * stride;
        fill_step(want[(size_t)b], ref.n[(size_t)b], ref.neff[(size_t)b], pred ? lin[(size_t)b] : 0.0, pred ? ang[(size_t)b] : 0.0,
                  (upd ? FLAG_UPDATE : 0) | (pred && p == 0 ? FLAG_PREDICT : 0), pidx ? pidx + off : nullptr, prange ? prange + off : nullptr,
                  pbearing ? pbearing + off : nullptr, upd && meas ? m[(size_t)b] : 0, p);
        want_pass_hi = std::max(want_pass_hi, want[(size_t)b].m);
        const StepIn& s = out[(size_t)b];
        CHECK(((s.flags & FLAG_PREDICT) != 0) == (pred && p == 0) && ((s.flags & FLAG_UPDATE) != 0) == upd, "trial %d: flags of pass %d", it, p);
        CHECK(g.neff[(size_t)b] >= before[(size_t)b] && g.neff[(size_t)b] <= g.n[(size_t)b] && s.neff == g.neff[(size_t)b], "trial %d: bound", it);
        CHECK(g.neff_enq[(size_t)b] == (g.opt_active_bound ? g.neff[(size_t)b] : g.n[(size_t)b]), "trial %d: the enqueued bound", it);
        for (int i = 0; i < s.m; ++i) got_idx[b].push_back(s.idx[i]);
      }
      CHECK(std::memcmp(out.data(), want.data(), sizeof(StepIn) * out.size()) == 0, "trial %d: pass %d differs from the plain loop", it, p);
      CHECK(pass_hi == want_pass_hi, "trial %d: pass %d holds %d, reported %d", it, p, want_pass_hi, pass_hi);
    }
    CHECK(g.neff == ref.neff, "trial %d: bounds differ from the plain loop", it);
    for (int b = 0; b < batch; ++b) {                    // every observation exactly once, in order
      const int mb = upd && meas ? m[(size_t)b] : 0;
      CHECK((int)got_idx[b].size() == mb, "trial %d: trajectory %d carries %zu of %d", it, b, got_idx[b].size(), mb);
      for (int i = 0; i < mb; ++i) CHECK(got_idx[b][(size_t)i] == idx[(size_t)b * stride + i], "trial %d: order", it);
    }
  }
  CHECK(refused > 1000 && accepted > 1000 && empty_null > 20 && update_only > 20, "coverage: %d refused, %d accepted, %d / %d", refused,
        accepted, empty_null, update_only);
}

// fill_det_records: exactly count[b] detections per trajectory out of the strided arrays, which end with the last trajectory's
// last detection (a read past count[b] there is a sanitizer report), nothing written past them.
static void check_det_records(std::mt19937& rng) {
  for (int it = 0; it < 2000; ++it) {
    const int batch = rng() % 2 ? 1 : 3;
    const int strides[] = {0, 1, 5, 40, DMAX}, stride = strides[rng() % 5];
    HostPlan h = bank(3 + 2 * 10, std::vector<int>((size_t)batch, 3 + 2 * 10));
    h.cfg.enable_measurement_model = 1;
    std::vector<int> count;
    for (int b = 0; b < batch; ++b) count.push_back(rng() % 4 == 0 ? 0 : (int)(rng() % (stride + 1)));
    const size_t len = (size_t)(batch - 1) * stride + count.back();
    std::vector<double> lin, ang, pose_t(3 * len), pose_err(len);
    std::vector<int> tag_id(len);
    for (int b = 0; b < batch; ++b) lin.push_back(0.01 * b + 0.001 * it), ang.push_back(-0.02 * b);
    for (size_t e = 0; e < len; ++e) {
      tag_id[e] = (int)(rng() % 50);
      pose_err[e] = 0.5 + e;
      for (int c = 0; c < 3; ++c) pose_t[3 * e + c] = 10.0 * e + c;
    }
    int m_hi = -1;
    CHECK(plan_det_windows(&h, lin.data(), ang.data(), count.data(), len ? tag_id.data() : nullptr, len ? pose_t.data() : nullptr,
                           len ? pose_err.data() : nullptr, stride, &m_hi) == nullptr && m_hi >= 0 && m_hi <= AMAX, "trial %d refused", it);
    std::vector<DetIn> out((size_t)batch);
    std::memset(out.data(), 0xAB, sizeof(DetIn) * out.size());
    DetIn untouched;
    std::memset(&untouched, 0xAB, sizeof untouched);
    fill_det_records(&h, lin.data(), ang.data(), count.data(), len ? tag_id.data() : nullptr, len ? pose_t.data() : nullptr,
                     len ? pose_err.data() : nullptr, stride, out.data());
    for (int b = 0; b < batch; ++b) {
      const DetIn& d = out[(size_t)b];
      CHECK(d.lin == lin[(size_t)b] && d.ang == ang[(size_t)b] && d.count == count[(size_t)b] && d.pad == 0, "trial %d: head of %d", it, b);
      for (int i = 0; i < DMAX; ++i) {
        const size_t e = (size_t)b * stride + i;
        if (i < count[(size_t)b])
          CHECK(d.tag_id[i] == tag_id[e] && d.pose_err[i] == pose_err[e] && d.pose_t[i][0] == pose_t[3 * e] && d.pose_t[i][1] == pose_t[3 * e + 1] &&
                    d.pose_t[i][2] == pose_t[3 * e + 2], "trial %d: detection %d of %d", it, i, b);
        else
          CHECK(d.tag_id[i] == untouched.tag_id[i] && std::memcmp(&d.pose_err[i], &untouched.pose_err[i], sizeof(double)) == 0 &&
                    std::memcmp(d.pose_t[i], untouched.pose_t[i], 3 * sizeof(double)) == 0, "trial %d: entry %d of %d was written", it, i, b);
      }
    }
  }
}

// The scaffold of the read-only queries and the log rings: bank_range_ok, pending_kb, plan_staging, ring_range_ok, ring_pieces.
static void check_scaffold(std::mt19937& rng) {
  // the range check against its plain statement, sums in 64 bits; counts near INT_MAX must not overflow
  const int edge[] = {INT_MIN, INT_MIN + 1, -7, -1, 0, 1, 2, 3, 4, 5, 6, 7, INT_MAX - 6, INT_MAX - 1, INT_MAX};
  for (int batch = 1; batch <= 6; ++batch) {
    HostPlan h;
    h.batch = batch;
    for (int b0 : edge)
      for (int count : edge) {
        bool inside = count >= 1;
        for (long long b = b0; inside && b < (long long)b0 + std::min(count, 8); ++b) inside = b >= 0 && b < batch;
        if (count > 8) inside = false;                 // (more trajectories than any bank here)
        CHECK(bank_range_ok(&h, b0, count) == inside, "batch %d range (%d, %d)", batch, b0, count);
      }
  }
  for (int k = 0; k <= KTOT; ++k) {
    HostPlan h;
    h.batch = 1;
    h.n = {3};
    h.neff_enq = {3};
    h.cu_count = 256;
    h.pending_k = k;
    CHECK(pending_kb(&h) == 4 * plan_pass(&h).nkt && pending_kb(&h) >= k && pending_kb(&h) < k + 4, "pending_kb(%d)", k);
  }
  // the staging layout: random tables ...
  for (int it = 0; it < 20000; ++it) {
    StagingPlan s;
    s.inputs = rng() % 3 == 0 ? 0 : rng() % 5000;
    const int nd = (int)(rng() % (STAGE_DSTS + 1));
    for (int i = 0; i < nd; ++i) s.add(rng() % 4 != 0, rng() % 3 == 0 ? 0 : (size_t)(rng() % 100000), rng() % 2 == 0);
    const size_t total = plan_staging(s);
    size_t sum = s.inputs, prev_end = s.inputs;
    for (int i = 0; i < nd; ++i) {
      const StagingPlan::Dst& d = s.dst[i];
      CHECK(d.staged == (d.present && d.words > 0 && !d.device), "destination %d staged %d", i, (int)d.staged);
      if (!d.staged) continue;
      CHECK(d.at == prev_end && d.at >= s.inputs && d.at + d.words <= total, "region %d [%zu, %zu) behind %zu of %zu", i, d.at,
            d.at + d.words, prev_end, total);           // (table order, back to back: disjoint)
      prev_end = d.at + d.words;
      sum += d.words;
    }
    CHECK(total == sum && total == prev_end, "total %zu, sum %zu", total, sum);
  }
  {                                                    // (arithmetic in size_t: two regions of 3 G doubles)
    StagingPlan s;
    s.add(true, (size_t)3 << 30, false);
    s.add(true, (size_t)3 << 30, false);
    CHECK(plan_staging(s) == (size_t)6 << 30 && s.dst[1].at == (size_t)3 << 30, "size_t arithmetic");
  }
  // ... and the three queries' tables against the sums their entry points formed by hand before they shared the planner
  for (int it = 0; it < 20000; ++it) {
    const size_t count = 1 + rng() % 40, stride = 1 + rng() % MMAX, cap = rng() % 3 == 0 ? 0 : rng() % 300;
    bool pin[STAGE_DSTS], have[STAGE_DSTS];
    for (int i = 0; i < STAGE_DSTS; ++i) {
      pin[i] = rng() % 2 == 0;
      have[i] = rng() % 3 != 0;
    }
    {                                                  // ekf_download_marginals(pose, landmarks): pose is never NULL
      const size_t mcap = have[1] ? cap : 0, pose_words = count * 9, lm_words = count * mcap * 4;
      StagingPlan s;
      s.add(true, pose_words, pin[0]);
      s.add(have[1], lm_words, pin[1]);
      CHECK(plan_staging(s) == (pin[0] ? 0 : pose_words) + (have[1] && !pin[1] ? lm_words : 0), "marginals layout");
    }
    {                                                  // ekf_associate: cand is never NULL, the full matrices come together
      const bool full = have[4];
      const size_t obs = count * stride, full_words = obs * (full ? cap : 0);
      const size_t m_words = (count + 1) / 2, part_words = count * (1 + rng() % 6) * stride * 8;
      const size_t words[STAGE_DSTS] = {obs, obs * 2, obs * 2, obs, full_words, full_words};
      const bool given[STAGE_DSTS] = {true, have[1], have[2], have[3], full, full};
      StagingPlan s;
      s.inputs = 2 * obs + m_words + part_words;
      size_t need = 2 * obs + m_words + part_words;
      for (int i = 0; i < STAGE_DSTS; ++i) {
        s.add(given[i], words[i], given[i] && words[i] && pin[i]);
        if (given[i] && words[i] && !pin[i]) need += words[i];
      }
      CHECK(plan_staging(s) == need, "associate layout");
    }
    {                                                  // ekf_download_joint(mean, cov): cov is never NULL
      const size_t ns = 3 + 2 * (1 + rng() % JMAX), nsp = (ns + JQ_TILE - 1) / JQ_TILE * JQ_TILE;
      const size_t sel_words = (count * 2 * nsp + 1) / 2, mean_words = count * ns, cov_words = mean_words * ns;
      StagingPlan s;
      s.inputs = sel_words;
      s.add(have[0], mean_words, pin[0]);
      s.add(true, cov_words, pin[1]);
      CHECK(plan_staging(s) == sel_words + (have[0] && !pin[0] ? mean_words : 0) + (pin[1] ? 0 : cov_words), "joint layout");
    }
  }
  // the rings: "among the last cap of the steps logged", stated step by step, and the pieces of a range
  for (int cap = 1; cap <= 5; ++cap)
    for (long long steps = 0; steps <= 12; ++steps)
      for (long long first = -2; first <= 14; ++first)
        for (int count = -1; count <= 7; ++count) {
          bool ok = count >= 0 && first >= 0;
          for (long long t = first; ok && t < first + count; ++t) ok = t < steps && t >= steps - cap;
          // (an empty range is held to the same window: it names a position, [first, first) with first in [steps - cap, steps])
          if (count == 0) ok = first >= 0 && first <= steps && first >= steps - cap;
          CHECK(ring_range_ok(first, count, steps, cap) == ok, "ring range (%lld, %d) of %lld, cap %d", first, count, steps, cap);
          if (!ok) continue;
          const RingPieces rp = ring_pieces(first, count, cap);
          CHECK(rp.n <= 2 && (rp.n > 0) == (count > 0), "%d pieces", rp.n);
          long done = 0;
          for (int i = 0; i < rp.n; ++i) {
            const RingPieces::Piece& c = rp.piece[i];
            CHECK(c.done == done && c.rows >= 1 && c.slot == (long)((first + done) % cap) && c.slot + c.rows <= cap,
                  "piece %d: slot %ld, %ld rows from %ld (cap %d)", i, c.slot, c.rows, c.done, cap);
            done += c.rows;
          }
          CHECK(done == count, "pieces cover %ld of %d", done, count);
        }
  CHECK(!ring_range_ok(LLONG_MAX - 1, 5, LLONG_MAX, 8) && ring_range_ok(LLONG_MAX - 5, 5, LLONG_MAX, 8), "ring range at the top");
  for (int it = 0; it < 20000; ++it) {                 // larger rings, random ranges inside the window
    const int cap = 1 + (int)(rng() % 1000);
    const long long steps = (long long)(rng() % 100000);
    const int count = (int)(rng() % (std::min<long long>(cap, steps) + 1));
    const long long lo = std::max<long long>(0, steps - cap), first = lo + (long long)(rng() % (steps - count - lo + 1));
    CHECK(ring_range_ok(first, count, steps, cap), "ring range (%lld, %d) of %lld, cap %d", first, count, steps, cap);
    const RingPieces rp = ring_pieces(first, count, cap);
    long done = 0;
    for (int i = 0; i < rp.n; ++i) {
      CHECK(rp.piece[i].done == done && rp.piece[i].slot == (long)((first + done) % cap) && rp.piece[i].rows >= 1 &&
            rp.piece[i].slot + rp.piece[i].rows <= cap, "piece %d", i);
      done += rp.piece[i].rows;
    }
    CHECK(rp.n <= 2 && done == count, "%d pieces cover %ld of %d", rp.n, done, count);
  }
}

int main() {
  std::mt19937 rng(20261004);
  check_layout();
  check_queues();
  check_shares(rng);
  check_planning(rng);
  check_launch_plans(rng);
  check_cadence_orders(rng);
  check_step_records(rng);
  check_obs_planner(rng);
  check_det_records(rng);
  check_scaffold(rng);
  std::printf("host_plan_check: %ld checks passed\n", checks);
  return 0;
}
