// Sanitizer build of the handle's ownership types (slam-duckietown_amd/csrc/ekf_resources.h, the same source the library ships):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DEKF_HOST_ONLY
//       -I slam-duckietown_amd/csrc tests/resources_check.cpp -o resources_check
// A counting backend stands in for the runtime: it logs every call, keeps the live allocations and events, knows which buffers
// work "in flight" on a stream still uses and which pinned copies an upload has not left yet, and can fail the k-th call.  The
// script below is the allocation script of an ekf_handle (ekf_api.hip): ekf_create's set, every first-use group, the two
// double-buffered uploads through several regrows, the noise upload twice in a row, the log rings resized up, down and to 0,
// reserve growing.  It is replayed once without a failure and once for every k up to its length with call k failing; the step
// that reports the failure is checked and retried, the rest of the script follows, the handle is torn down as free_all does.
// Asserted: nothing live at the end and no double free; a failed group leaves every member empty and its retry succeeds; a
// buffer is never freed while a stream still uses it; a pinned copy is never handed out between a commit and the wait for that
// commit's event; every group reports "new" exactly once per allocation.  tests/test_cpu_host.py builds and runs it (CPU only).
// The input ring (InputRing) is driven in the order the step entries drive it, both paths mixed: a pinned slot is never handed
// out between its upload (staged path) or its launch (direct path) and the wait for its group's event, a take behind a failed
// call waits for the stream once and the ring goes on.
// Only the TYPES are under test here: ring_resize and upload below restate what the call sites of ekf_api.hip do with them and
// share no code with them, so a call site that drifted (no release before the new ring, the wrong copy of a pair) is not seen
// here -- the call sites are covered by the GPU tests (tests/test_gpu_cadence.py::test_run_plan_copies_regrow_on_one_handle,
// tests/test_gpu_api_regressions.py::test_handle_churn_leaves_nothing_behind, the log and noise suites).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "ekf_resources.h"
#include "plan_check.h"

// ---- the counting backend ----
struct Call {
  const char* name;
  const void* a;
  long b;
};
struct World {
  std::vector<Call> log;
  long calls = 0, fail_at = -1;
  bool failed = false;                                 // the injected failure has happened
  std::set<void*> device, pinned;
  std::map<const void*, size_t> extent;                // allocation -> its bytes
  std::set<int> events;
  int next_event = 1;
  std::map<const void*, int> used_on;                  // buffer -> stream whose work in flight uses it
  std::map<const void*, int> upload_event;             // pinned copy -> event behind the upload that still reads it
  std::map<const void*, int> upload_bare;              // pinned copy -> stream of an upload with no event behind it (yet)
  std::map<int, int> recorded_on;                      // event (recorded, not yet waited for) -> stream
};
static World* W = nullptr;

struct CountingBackend {
  using Stream = int;
  using Event = int;
  static constexpr unsigned pinned_default = 0;
  static constexpr int ERR = 2;
  // True when this call is the one to fail.  Releases (frees, event destruction) report the error after they have released:
  // what a runtime that failed there has kept cannot be known, and nothing could be done about it.
  static bool hit(const char* name, const void* a, long b) {
    W->log.push_back({name, a, b});
    const bool fail = W->calls++ == W->fail_at;
    if (fail) W->failed = true;
    return fail;
  }
  static void stream_done(int st) {
    for (auto it = W->used_on.begin(); it != W->used_on.end();) it = it->second == st ? W->used_on.erase(it) : ++it;
    for (auto it = W->upload_bare.begin(); it != W->upload_bare.end();) it = it->second == st ? W->upload_bare.erase(it) : ++it;
    for (auto it = W->recorded_on.begin(); it != W->recorded_on.end();)
      if (it->second == st) {
        event_done(it->first);
        it = W->recorded_on.erase(it);
      } else {
        ++it;
      }
  }
  static bool uploading(const void* pinned) { return W->upload_event.count(pinned) + W->upload_bare.count(pinned) > 0; }
  static void event_done(int ev) {
    for (auto it = W->upload_event.begin(); it != W->upload_event.end();) it = it->second == ev ? W->upload_event.erase(it) : ++it;
  }
  static int alloc(std::set<void*>& live, const char* name, void** p, size_t bytes) {
    if (hit(name, nullptr, (long)bytes)) return ERR;
    CHECK(bytes > 0, "%s of 0 bytes", name);
    *p = std::malloc(bytes);
    std::memset(*p, 0xAB, bytes);
    live.insert(*p);
    W->extent[*p] = bytes;
    return 0;
  }
  // [p, p + bytes) lies inside one live allocation of `live` (the ring's slots are parts of their buffers)
  static bool inside(const std::set<void*>& live, const void* p, size_t bytes) {
    auto it = W->extent.upper_bound(p);
    if (it == W->extent.begin()) return false;
    --it;
    const char *base = static_cast<const char*>(it->first), *q = static_cast<const char*>(p);
    return live.count(const_cast<void*>(it->first)) == 1 && q + bytes <= base + it->second;
  }
  static int release(std::set<void*>& live, const char* name, void* p) {
    const bool fail = hit(name, p, 0);
    CHECK(live.count(p) == 1, "%s of %p: not live (double free?)", name, p);
    CHECK(W->used_on.count(p) == 0, "%s of %p while stream %d still uses it", name, p, W->used_on[p]);
    CHECK(!uploading(p), "%s of %p while its upload has not run", name, p);
    live.erase(p);
    W->extent.erase(p);
    std::free(p);
    return fail ? ERR : 0;
  }
  static int device_alloc(void** p, size_t bytes) { return alloc(W->device, "device_alloc", p, bytes); }
  static int device_free(void* p) { return release(W->device, "device_free", p); }
  static int pinned_alloc(void** p, size_t bytes, unsigned flag) {
    CHECK(flag == 0 || flag == 7, "flag %u", flag);
    return alloc(W->pinned, "pinned_alloc", p, bytes);
  }
  static int pinned_free(void* p) { return release(W->pinned, "pinned_free", p); }
  static int event_create(Event* e, bool timing) {
    if (hit("event_create", nullptr, timing)) return ERR;
    *e = W->next_event++;
    W->events.insert(*e);
    return 0;
  }
  static int event_destroy(Event e) {
    const bool fail = hit("event_destroy", nullptr, e);
    CHECK(W->events.erase(e) == 1, "event %d destroyed twice", e);
    return fail ? ERR : 0;
  }
  static int event_record(Event e, Stream st) {
    if (hit("event_record", nullptr, e)) return ERR;
    CHECK(W->events.count(e) == 1, "record of event %d", e);
    event_done(e);                                     // (a new record replaces the old one)
    W->recorded_on[e] = st;
    // (stream order: the event is behind every upload enqueued on the stream so far, not only the last one)
    for (auto it = W->upload_bare.begin(); it != W->upload_bare.end();)
      if (it->second == st) {
        W->upload_event[it->first] = e;
        it = W->upload_bare.erase(it);
      } else {
        ++it;
      }
    return 0;
  }
  static int event_wait(Event e) {
    if (hit("event_wait", nullptr, e)) return ERR;
    CHECK(W->events.count(e) == 1, "wait for event %d", e);
    event_done(e);
    W->recorded_on.erase(e);
    return 0;
  }
  static int stream_wait(Stream st) {
    if (hit("stream_wait", nullptr, st)) return ERR;
    stream_done(st);
    return 0;
  }
  static int copy_to_device(void* dst, const void* src, size_t bytes, Stream st) {
    if (hit("copy_to_device", src, (long)bytes)) return ERR;
    CHECK(inside(W->device, dst, bytes) && inside(W->pinned, src, bytes), "copy %p <- %p", dst, src);
    std::memcpy(dst, src, bytes);                      // (the sanitizer checks both capacities)
    W->used_on[dst] = st;
    W->upload_event.erase(src);
    W->upload_bare[src] = st;                          // (until the event behind it is recorded only the stream can be waited for)
    return 0;
  }
};

using namespace ekf::res;
using B = CountingBackend;
template <class T> using DBuf = DeviceBuf<T, B>;
template <class T> using PBuf = PinnedBuf<T, B>;
template <class T> using Staged = StagedUpload<T, B>;
using Ev = Event<B>;

// Work enqueued on `st` reads or writes the buffer.
template <class Buf> static void in_flight(const Buf& b, int st) {
  if (b.p) W->used_on[b.p] = st;
}

// ---- the handle: one member per kind of thing ekf_handle owns ----
constexpr int STREAM = 1, AUX = 2, BATCH = 2, RING = 16;
struct Handle {
  // ekf_create's set
  DBuf<double> dP, dmu2[2], dV;
  DBuf<int> dn;
  DBuf<long> d_ring;
  PBuf<long> h_ring;
  PBuf<unsigned> h_flags;
  PBuf<double> h_pack{7};                              // (the one allocated with a flag of its own, on first use)
  Ev ev_fork, ev_pass, t0, t1;
  InputRing<B, RING, 4> ring;                          // (the slots of h_ring / d_ring)
  std::vector<Ev> prof_pool;
  // first-use groups
  DBuf<int> dtagmap, dneff;
  DBuf<long> d_det, d_assoc_step, d_assoc_out;
  PBuf<long> h_det;
  DBuf<int> drm_tab;
  DBuf<unsigned> drm_flag;
  DBuf<double> dF, dQ, dTmp;
  DBuf<long> dcad2[2];
  DBuf<double> dprow3[2], dxg, dbg, dgmu;
  DBuf<unsigned> dsync;
  DBuf<long> dpre[2];
  DBuf<double> dgbuf, dgate, dfront, dcolbuf;
  DBuf<double> lone, with_b, with_c;                   // a group whose first member exists before the group is asked for
  // stream-ordered uploads
  Staged<int> shares2[2];
  Staged<long> plan2[2];
  Staged<double> noise;
  int shares_cur = 0, plan_cur = 0;
  // the log rings, the buffers that only grow
  DBuf<double> dpose;
  DBuf<long> dinnov;
  DBuf<int> dinnov_m;
  DBuf<double> dquery;
  DBuf<long> d_stream;
};

struct Step {
  std::string name;
  std::function<Status(Handle&)> run;
  std::function<void(Handle&)> after_failure;          // what must hold when `run` reported a failure (may be empty)
};
static std::map<std::string, int> fresh_reports;

template <class... Bufs> static bool all_empty(const Bufs&... b) { return (... && (b.p == nullptr && b.cap == 0)); }
template <class... Bufs> static bool all_live(const Bufs&... b) { return (... && (b.p != nullptr && b.cap > 0)); }

// A first-use group, as its site in ekf_api.hip ensures it: "new" exactly when a member was missing; a failed call leaves every
// member as it was before the call.  `disjoint`: no member belongs to another group too, so the group is all there or not at all.
template <class Live, class Ensure> static Step group_step(const std::string& label, bool disjoint, Live live, Ensure ensure) {
  Step s;
  s.name = label;
  s.run = [=](Handle& h) {
    const std::vector<bool> before = live(h);
    const bool was_complete = std::count(before.begin(), before.end(), true) == (long)before.size();
    if (disjoint) CHECK(was_complete || std::count(before.begin(), before.end(), true) == 0, "%s: half allocated", label.c_str());
    bool fresh = true;
    const Status st = ensure(h, &fresh);
    const std::vector<bool> after = live(h);
    if (st.ok()) {
      CHECK(std::count(after.begin(), after.end(), true) == (long)after.size(), "%s: not complete behind a successful call", label.c_str());
      CHECK(fresh == !was_complete, "%s: fresh = %d for a group that was %s", label.c_str(), (int)fresh, was_complete ? "complete" : "not");
      if (fresh) fresh_reports[label] += 1;
    } else {
      CHECK(!fresh, "%s: a failed call reported a new group", label.c_str());
      CHECK(st.err == B::ERR, "%s: error code %d", label.c_str(), st.err);
      CHECK(after == before, "%s: a failed call must release what it allocated, and nothing else", label.c_str());
      if (disjoint) CHECK(std::count(after.begin(), after.end(), true) == 0, "%s: a failed group leaves every member empty", label.c_str());
    }
    return st;
  };
  return s;
}
#define MEMBERS(...) [](Handle& h) { return live_of(__VA_ARGS__); }
template <class... Bufs> static std::vector<bool> live_of(const Bufs&... b) { return {(b.p != nullptr && b.cap > 0)...}; }

// ring_resize of ekf_api.hip: the old ring is released once the stream is idle, then the new one is ensured as a group.
template <class... Bufs> static Status ring_resize(const std::string& label, int capacity, Want<Bufs>... arrays) {
  (in_flight(*arrays.buf, STREAM), ...);               // (launches in flight still write the old ring)
  if (Status s = release_group<B>(STREAM, *arrays.buf...); !s.ok()) return s;
  CHECK(all_empty(*arrays.buf...), "%s: released", label.c_str());
  if (capacity == 0) return {};
  bool fresh = true;
  const size_t rows = (size_t)capacity * BATCH;
  const Status st = ensure_group(&fresh, want(*arrays.buf, rows * arrays.n)...);
  if (st.ok()) {
    CHECK(fresh && all_live(*arrays.buf...), "%s: capacity %d", label.c_str(), capacity);
    CHECK((... && (arrays.buf->cap == rows * arrays.n)), "%s: sizes", label.c_str());
    fresh_reports[label] += 1;
  } else {
    CHECK(!fresh && all_empty(*arrays.buf...), "%s: a failed resize leaves the log off", label.c_str());
  }
  return st;
}

// One upload through a double-buffered pair, as flush_pending / upload_run_plan do it: the copy not in use is rewritten.
template <class T> static Status upload(Staged<T> (&pair)[2], int* cur, size_t count, size_t at_least, int st) {
  const int nb = *cur ^ 1;
  Staged<T>& u = pair[nb];
  const size_t cap_before = u.dev.cap;
  const T *dev_before = u.dev.p, *host_before = u.host.p;
  T* stage = nullptr;
  bool fresh = false;
  const Status s = u.begin(count, at_least, st, &stage, &fresh);
  if (!s.ok()) {
    CHECK((u.dev.p == dev_before && u.host.p == host_before && u.dev.cap == cap_before) || all_empty(u.dev, u.host),
          "a failed begin leaves the pair as it was or empty");
    return s;
  }
  CHECK(stage == u.host.p && stage != nullptr, "begin hands out the pinned copy");
  CHECK(u.dev.cap >= count && u.host.cap == u.dev.cap, "room for %zu: %zu / %zu", count, u.dev.cap, u.host.cap);
  CHECK(fresh == (cap_before < count || dev_before == nullptr), "fresh");
  if (fresh) CHECK(u.dev.cap == std::max(count, at_least), "a new pair holds max(count, at_least)");
  CHECK(!B::uploading(stage), "the pinned copy was handed out while its last upload had not run");
  for (size_t i = 0; i < count; ++i) stage[i] = (T)(i + 1);
  if (Status c = u.commit(count, st); !c.ok()) {
    CHECK(W->upload_bare.count(stage) == 0, "a failed commit leaves no upload in flight that no event is behind");
    return c;
  }
  CHECK(u.device() == u.dev.p && u.device()[count - 1] == (T)count, "the device copy holds the table");
  CHECK(W->upload_event.count(stage) == 1 && W->upload_event[stage] == u.done.ev, "the upload is behind the pair's event");
  *cur = nb;
  return {};
}

static std::vector<Step> script() {
  std::vector<Step> s;
  auto single = [&](const std::string& label, std::function<Status(Handle&)> f) { s.push_back({label, std::move(f), nullptr}); };
  // ---- ekf_create: its events and buffers one by one (a failure there ends in free_all: the teardown below) ----
  single("create", [](Handle& h) {
    for (Ev* e : {&h.ev_fork, &h.ev_pass})
      if (Status st = e->ensure(); !st.ok()) return st;
    if (Status st = h.dP.ensure(4096 * BATCH); !st.ok()) return st;
    for (auto& m : h.dmu2)
      if (Status st = m.ensure(64 * BATCH); !st.ok()) return st;
    if (Status st = h.dV.ensure(64 * 80 * BATCH); !st.ok()) return st;
    if (Status st = h.dn.ensure(BATCH); !st.ok()) return st;
    if (Status st = h.d_ring.ensure(BATCH * RING); !st.ok()) return st;
    if (Status st = h.h_ring.ensure(BATCH * RING); !st.ok()) return st;
    if (Status st = h.h_flags.ensure(BATCH); !st.ok()) return st;
    if (Status st = h.ring.ensure(); !st.ok()) return st;
    if (Status st = h.t0.ensure(true); !st.ok()) return st;
    return h.t1.ensure(true);
  });
  // ---- the step ring's events: recorded per group of slots, waited for only once recorded ----
  single("ring events", [](Handle& h) {
    for (int round = 0; round < 2; ++round)
      for (auto& e : h.ring.ev) {
        const long before = W->calls;
        const bool recorded = e.recorded;
        if (Status st = e.wait_if_recorded(); !st.ok()) return st;
        CHECK((W->calls > before) == recorded, "an event is waited for exactly when it has been recorded");
        if (Status st = e.record(STREAM); !st.ok()) return st;
        CHECK(e.recorded, "record sets the bit");
      }
    return Status{};
  });
  // ---- the input ring itself, as the step entries of ekf_api.hip drive it: 3 x RING calls of take, fill, submit, launch,
  //      launched, the staged and the direct order mixed.  A call that fails returns at once (the entry's early return); the
  //      retry goes on from wherever the ring stands, with the failed call's group left open ----
  single("input ring", [](Handle& h) {
    for (int i = 0; i < 3 * RING; ++i) {
      const bool direct = i % 3 == 1;
      const int s = h.ring.pos, g = s / 4;
      const bool was_open = h.ring.open[g], recorded = h.ring.ev[g].recorded;
      const long before = W->calls;
      int slot = -1;
      if (Status st = h.ring.take(STREAM, &slot); !st.ok()) {
        CHECK(h.ring.pos == s && h.ring.open[g] == was_open, "a failed take leaves the ring where it was");
        return st;
      }
      CHECK(slot == s && h.ring.pos == (s + 1) % RING && h.ring.open[g], "slots are handed out in order: %d at %d", slot, s);
      const std::string waited = W->calls > before ? W->log[(size_t)before].name : "";
      if (s % 4 != 0) CHECK(W->calls == before, "inside a group nothing is waited for");
      else if (was_open) CHECK(W->calls == before + 1 && waited == "stream_wait", "a group a failed call left open: the stream is waited for, once");
      else CHECK(W->calls == before + (recorded ? 1 : 0) && (!recorded || waited == "event_wait"), "the group's event is waited for, if recorded");
      long *hs = h.h_ring.p + (size_t)slot * BATCH, *ds = h.d_ring.p + (size_t)slot * BATCH;
      CHECK(!B::uploading(hs), "slot %d was handed out while the work that reads it had not run", slot);
      for (int b = 0; b < BATCH; ++b) hs[b] = 100L * i + b;
      if (Status st = h.ring.submit(slot, direct, ds, hs, sizeof(long) * BATCH, STREAM); !st.ok()) {
        CHECK(h.ring.open[g], "a failed submit leaves the group open");
        return st;
      }
      if (direct) W->upload_bare[hs] = STREAM;           // the launch marker: a kernel on the stream reads the pinned slot itself
      else CHECK(ds[BATCH - 1] == 100L * i + BATCH - 1 && B::uploading(hs), "the staged path copies the slot");
      in_flight(h.d_ring, STREAM);
      if (Status st = h.ring.launched(slot, direct, STREAM); !st.ok()) {
        CHECK(h.ring.open[g], "a failed record leaves the group open");
        return st;
      }
      if (slot % 4 == 3)
        CHECK(!h.ring.open[g] && W->upload_event.count(hs) == 1 && W->upload_event[hs] == h.ring.ev[g].ev,
              "the group's event is behind the work that read its last slot");
    }
    return Status{};
  });
  // ---- first-use allocations ----
  single("h_pack", [](Handle& h) {
    for (int i = 0; i < 2; ++i)
      if (Status st = h.h_pack.ensure(1000); !st.ok()) return st;
    CHECK(h.h_pack.cap == 1000, "ensure allocates once");
    return Status{};
  });
  for (int round = 0; round < 2; ++round) {            // (every group twice: the second call finds it complete)
    s.push_back(group_step("association", true, MEMBERS(h.dtagmap, h.dneff, h.d_det, h.h_det, h.d_assoc_step, h.d_assoc_out),
                           [](Handle& h, bool* fresh) {
                             return ensure_group(fresh, want(h.dtagmap, 1024 * BATCH), want(h.dneff, BATCH), want(h.d_det, BATCH * RING),
                                                 want(h.h_det, BATCH * RING), want(h.d_assoc_step, BATCH * 2), want(h.d_assoc_out, BATCH));
                           }));
    s.push_back(group_step("removal", true, MEMBERS(h.drm_tab, h.drm_flag), [](Handle& h, bool* fresh) {
      return ensure_group(fresh, want(h.drm_tab, 2 * 64), want(h.drm_flag, 64 * BATCH));
    }));
    s.push_back(group_step("dense", true, MEMBERS(h.dF, h.dQ, h.dTmp), [](Handle& h, bool* fresh) {
      *fresh = !all_live(h.dF, h.dQ, h.dTmp);          // (this site has nothing to initialise and passes no `fresh`)
      const Status st = ensure_group(nullptr, want(h.dF, 4096), want(h.dQ, 4096), want(h.dTmp, 4096));
      if (!st.ok()) *fresh = false;
      return st;
    }));
    s.push_back(group_step("cadence records", true, MEMBERS(h.dcad2[0], h.dcad2[1]), [](Handle& h, bool* fresh) {
      return ensure_group(fresh, want(h.dcad2[0], BATCH), want(h.dcad2[1], BATCH));
    }));
    // (the chained set shares the records with the group above and the block buffer with the look-ahead, which allocates it alone)
    s.push_back(group_step("chained run", false,
                           MEMBERS(h.dcad2[0], h.dcad2[1], h.dgbuf, h.dprow3[0], h.dprow3[1], h.dxg, h.dbg, h.dsync, h.dpre[0], h.dpre[1], h.dgmu),
                           [](Handle& h, bool* fresh) {
                             return ensure_group(fresh, want(h.dcad2[0], BATCH), want(h.dcad2[1], BATCH), want(h.dgbuf, 84 * 88 * BATCH),
                                                 want(h.dprow3[0], 3 * 64 * BATCH), want(h.dprow3[1], 3 * 64 * BATCH),
                                                 want(h.dxg, 84 * 88 * BATCH), want(h.dbg, 84 * 88 * BATCH), want(h.dsync, 8),
                                                 want(h.dpre[0], BATCH), want(h.dpre[1], BATCH), want(h.dgmu, 128 * BATCH));
                           }));
    single("single buffers", [](Handle& h) {
      if (Status st = h.dgbuf.ensure(84 * 88 * BATCH); !st.ok()) return st;
      if (Status st = h.dgate.ensure(BATCH); !st.ok()) return st;
      if (Status st = h.dfront.reserve(100 * BATCH, 0, STREAM); !st.ok()) return st;
      return h.dcolbuf.ensure(83 * 64 * BATCH);
    });
  }
  // ---- "new" is judged on the whole group: its first member may exist already (a buffer another site allocates too) ----
  s.push_back({"group behind its first member",
               [](Handle& h) {
                 if (Status st = h.lone.ensure(10); !st.ok()) return st;
                 const bool rest_empty = all_empty(h.with_b, h.with_c);
                 bool fresh = !rest_empty;
                 const Status st = ensure_group(&fresh, want(h.lone, 10), want(h.with_b, 20), want(h.with_c, 30));
                 if (st.ok()) CHECK(fresh == rest_empty && all_live(h.lone, h.with_b, h.with_c), "the rest is allocated and reported new");
                 else CHECK(!fresh, "a failed call reports nothing new");
                 return st;
               },
               [](Handle& h) { CHECK(all_empty(h.with_b, h.with_c), "what the failed call allocated is released; the rest stays as it was"); }});
  // ---- the share table: one size, alternately on either stream ----
  for (int i = 0; i < 5; ++i)
    single("share table", [i](Handle& h) { return upload(h.shares2, &h.shares_cur, 256 * 16 * 4, 0, i & 1 ? AUX : STREAM); });
  // ---- the run plan: pieces of 68, 68, 84 cadences against the first room of 64 per trajectory, then smaller and larger ----
  for (size_t cadences : {8, 68, 68, 84, 3, 200, 200, 64, 201})
    single("run plan", [cadences](Handle& h) {
      const Status st = upload(h.plan2, &h.plan_cur, cadences * BATCH, (size_t)64 * BATCH, STREAM);
      if (st.ok()) in_flight(h.plan2[h.plan_cur].dev, STREAM);    // (the run's kernels read the device copy)
      return st;
    });
  // ---- the noise table, set twice in a row and once more: one copy, so every call after the first waits for its event ----
  for (int i = 0; i < 3; ++i)
    single("noise table", [i](Handle& h) {
      double* stage = nullptr;
      const long before = W->calls;
      const bool exists = h.noise.dev.p != nullptr, recorded = h.noise.done.recorded;
      if (Status st = h.noise.begin(5 * BATCH, 0, STREAM, &stage); !st.ok()) return st;
      if (exists) CHECK(W->calls == before + (recorded ? 1 : 0), "no allocation, and a wait exactly when an upload was recorded");
      if (exists && recorded) CHECK(std::string(W->log.back().name) == "event_wait", "the wait is for the event");
      CHECK(!B::uploading(stage), "the staging copy is free");
      for (int j = 0; j < 5 * BATCH; ++j) stage[j] = i + j;
      return h.noise.commit(5 * BATCH, STREAM);
    });
  // ---- the log rings: up, down, off, on again ----
  for (int capacity : {5, 3, 0, 0, 4})
    single("pose log", [capacity](Handle& h) { return ring_resize("pose log", capacity, want(h.dpose, 12)); });
  for (int capacity : {5, 3, 0, 2})
    s.push_back({"innovation log", [capacity](Handle& h) { return ring_resize("innovation log", capacity, want(h.dinnov, 16), want(h.dinnov_m, 1)); },
                 [](Handle& h) { CHECK(all_empty(h.dinnov, h.dinnov_m) || all_live(h.dinnov, h.dinnov_m), "both arrays or neither"); }});
  // ---- buffers that only grow: the stream is waited for before the old one is freed, and only then ----
  for (size_t need : {10, 5, 100, 100, 40, 1000})
    single("reserve", [need](Handle& h) {
      for (int which = 0; which < 2; ++which) {
        const size_t cap_before = which ? h.d_stream.cap : h.dquery.cap;
        const void* p_before = which ? (void*)h.d_stream.p : (void*)h.dquery.p;
        const long before = W->calls;
        const Status st = which ? h.d_stream.reserve(need, 0, STREAM) : h.dquery.reserve(need, 32, STREAM);
        const size_t cap = which ? h.d_stream.cap : h.dquery.cap;
        const void* p = which ? (void*)h.d_stream.p : (void*)h.dquery.p;
        if (!st.ok()) {
          CHECK((p == p_before && cap == cap_before) || (p == nullptr && cap == 0), "a failed reserve: as it was or empty");
          return st;
        }
        if (need <= cap_before) {
          CHECK(W->calls == before && p == p_before, "enough room: nothing happens");
        } else {
          CHECK(cap == std::max(need, which ? (size_t)0 : (size_t)32), "grown to max(need, at_least): %zu", cap);
          if (p_before) CHECK(std::string(W->log[(size_t)before].name) == "stream_wait", "the stream is waited for first");
        }
        if (which) in_flight(h.d_stream, STREAM); else in_flight(h.dquery, STREAM);
      }
      return Status{};
    });
  // ---- the profiling pool: a vector of events that grows (events move, none is destroyed twice) ----
  single("profiling pool", [](Handle& h) {
    while (h.prof_pool.size() < 40) {
      Ev e;
      if (Status st = e.ensure(true); !st.ok()) return st;
      h.prof_pool.push_back(std::move(e));
    }
    return Status{};
  });
  return s;
}

// free_all: both streams idle, then the members release (nothing may fail the check for buffers still in use).
static void teardown(Handle* h) {
  W->fail_at = -1;
  CHECK(B::stream_wait(STREAM) == 0 && B::stream_wait(AUX) == 0, "teardown");
  delete h;
  CHECK(W->device.empty() && W->pinned.empty() && W->events.empty(), "live at the end: %zu device, %zu pinned, %zu events",
        W->device.size(), W->pinned.size(), W->events.size());
}

// One replay; call `fail_at` fails (-1: none).  Returns the number of backend calls the script made without the teardown.
static long replay(const std::vector<Step>& steps, long fail_at) {
  World world;
  W = &world;
  world.fail_at = fail_at;
  fresh_reports.clear();
  Handle* h = new Handle();
  int failures = 0;
  bool completed = true;
  for (const Step& step : steps) {
    Status st = step.run(*h);
    if (!st.ok()) {
      CHECK(world.failed && failures == 0, "%s reported a failure that was not injected (call %ld)", step.name.c_str(), fail_at);
      failures += 1;
      if (step.after_failure) step.after_failure(*h);
      if (step.name == "create") {                     // (ekf_create gives up: free_all)
        completed = false;
        break;
      }
      world.fail_at = -1;
      st = step.run(*h);                               // the caller tries again
      CHECK(st.ok(), "%s: the retry after failed call %ld failed", step.name.c_str(), fail_at);
    }
  }
  if (fail_at >= 0) CHECK(world.failed && failures == 1, "call %ld failed and nobody reported it", fail_at);
  const long calls = world.calls;
  if (completed) {                                     // one "new" per allocation: the groups once, the rings once per capacity > 0
    for (const char* g : {"association", "removal", "dense", "cadence records", "chained run"})
      CHECK(fresh_reports[g] == 1, "%s reported new %d times for one allocation", g, fresh_reports[g]);
    CHECK(fresh_reports["pose log"] == 3 && fresh_reports["innovation log"] == 3, "the rings: %d, %d", fresh_reports["pose log"],
          fresh_reports["innovation log"]);
  }
  teardown(h);
  W = nullptr;
  return calls;
}

int main() {
  const std::vector<Step> steps = script();
  const long length = replay(steps, -1);
  CHECK(length > 150, "the script makes %ld backend calls", length);
  for (long k = 0; k < length; ++k) replay(steps, k);
  std::printf("resources_check: %ld backend calls in the script, replayed with each of them failing; %ld checks passed\n", length,
              checks);
  return 0;
}
