// Ownership of what a handle holds on the device: device buffers, pinned host buffers, events, and the stream-ordered upload
// built from the three.  Every type is non-copyable and releases in its destructor, so a handle that is deleted (while its
// device is selected) frees everything it has, whatever was added to it since.  Plain C++17 with no HIP header: the types reach
// the runtime only through a backend struct B (template parameter) of static functions, each returning 0 or the runtime's error
// code:
//   B::Stream, B::Event (native handles), B::pinned_default (allocation flag)
//   device_alloc(void**, bytes) / device_free(void*)           pinned_alloc(void**, bytes, flag) / pinned_free(void*)
//   event_create(Event*, timing) / event_destroy(Event) / event_record(Event, Stream) / event_wait(Event)
//   stream_wait(Stream)                                        copy_to_device(void* dst, const void* src, bytes, Stream)
// ekf_api.hip supplies the HIP backend; tests/resources_check.cpp a counting one that can fail any call, and replays the
// handle's allocation script under -fsanitize=address,undefined (tests/test_cpu_host.py builds and runs it, -DEKF_HOST_ONLY).
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>

namespace ekf {
namespace res {

// What an operation reports: err = 0, or the backend's error code and the bytes the failed allocation asked for (0: no allocation).
struct Status {
  int err = 0;
  size_t bytes = 0;
  bool ok() const { return err == 0; }
};

// `cap` elements of device memory at p (nullptr: empty).
template <class T, class B> struct DeviceBuf {
  T* p = nullptr;
  size_t cap = 0;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { (void)reset(); }
  // Allocated on first use: n elements unless the buffer exists.
  Status ensure(size_t n) {
    if (p) return {};
    void* q = nullptr;
    if (int e = B::device_alloc(&q, sizeof(T) * n)) return {e, sizeof(T) * n};
    p = static_cast<T*>(q);
    cap = n;
    return {};
  }
  // Room for `need` elements (a new buffer holds at least `at_least`); only grows, the contents are not kept.  The old buffer
  // may still be in use by work in flight on `st`, which is waited for before it is freed.  A failed call leaves the buffer as
  // it was or empty.
  Status reserve(size_t need, size_t at_least, typename B::Stream st) {
    if (need <= cap) return {};
    if (p)
      if (int e = B::stream_wait(st)) return {e, 0};
    if (Status s = reset(); !s.ok()) return s;
    return ensure(std::max(need, at_least));
  }
  Status reset() {
    cap = 0;
    if (T* old = std::exchange(p, nullptr))
      if (int e = B::device_free(old)) return {e, 0};
    return {};
  }
};

// The same in pinned host memory, allocated with `flag`.
template <class T, class B> struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  unsigned flag = B::pinned_default;
  PinnedBuf() = default;
  explicit PinnedBuf(unsigned flag_) : flag(flag_) {}
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { (void)reset(); }
  Status ensure(size_t n) {
    if (p) return {};
    void* q = nullptr;
    if (int e = B::pinned_alloc(&q, sizeof(T) * n, flag)) return {e, sizeof(T) * n};
    p = static_cast<T*>(q);
    cap = n;
    return {};
  }
  Status reset() {
    cap = 0;
    if (T* old = std::exchange(p, nullptr))
      if (int e = B::pinned_free(old)) return {e, 0};
    return {};
  }
};

// An event, created on first use (ensure, or the first record), that knows whether it has been recorded.
template <class B> struct Event {
  typename B::Event ev{};
  bool made = false, recorded = false;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : ev(o.ev), made(std::exchange(o.made, false)), recorded(std::exchange(o.recorded, false)) {}
  ~Event() {
    if (made) (void)B::event_destroy(ev);
  }
  Status ensure(bool timing = false) {
    if (made) return {};
    if (int e = B::event_create(&ev, timing)) return {e, 0};
    made = true;
    return {};
  }
  Status record(typename B::Stream st) {
    if (Status s = ensure(); !s.ok()) return s;
    if (int e = B::event_record(ev, st)) return {e, 0};
    recorded = true;
    return {};
  }
  // The host waits for the last record; nothing to wait for before the first one.
  Status wait_if_recorded() {
    if (recorded)
      if (int e = B::event_wait(ev)) return {e, 0};
    return {};
  }
};

// ---- groups: several buffers that exist together or not at all ----
// A member of a group: the buffer and the elements it is to hold.
template <class Buf> struct Want {
  Buf* buf;
  size_t n;
};
template <class Buf> Want<Buf> want(Buf& buf, size_t n) { return {&buf, n}; }

// Every member exists.
template <class... Bufs> bool complete(Want<Bufs>... members) { return (... && (members.buf->p != nullptr)); }

// Ensures every member.  A group that was complete is left alone (*fresh = false); otherwise the missing members are allocated
// and *fresh = true says, once per allocation, that the caller has the group's contents to initialise (fresh may be nullptr:
// nothing to initialise).  On a failure whatever this call allocated is released again -- a group never stays half allocated
// -- and *fresh is false.
template <class... Bufs> Status ensure_group(bool* fresh, Want<Bufs>... members) {
  if (fresh) *fresh = false;
  if (complete(members...)) return {};
  constexpr size_t count = sizeof...(Bufs);
  bool mine[count] = {};
  Status st;
  size_t i = 0;
  auto alloc = [&](auto m) {
    const size_t at = i++;
    if (!st.ok() || m.buf->p) return;
    st = m.buf->ensure(m.n);
    mine[at] = st.ok();
  };
  (alloc(members), ...);
  if (st.ok()) {
    if (fresh) *fresh = true;
    return st;
  }
  i = 0;
  auto undo = [&](auto m) {
    if (mine[i++]) (void)m.buf->reset();
  };
  (undo(members), ...);
  return st;
}

// Empties every buffer; work in flight on `st` may still use them, so the stream is waited for first if any of them exists.
template <class B, class... Bufs> Status release_group(typename B::Stream st, Bufs&... bufs) {
  if ((... || (bufs.p != nullptr)))
    if (int e = B::stream_wait(st)) return {e, 0};
  Status out;
  auto drop = [&](auto& b) {
    const Status s = b.reset();
    if (out.ok()) out = s;
  };
  (drop(bufs), ...);
  return out;
}

// A table the host rewrites and the device reads: a pinned copy, a device copy and the event behind the last upload out of the
// pinned copy.  begin() makes room and hands out the pinned copy once that upload has been executed; commit() enqueues the copy
// on the stream -- no host synchronisation -- and records the event.  Two of them used alternately let the host build the next
// table while launches that read the previous one are still in flight.
template <class T, class B> struct StagedUpload {
  PinnedBuf<T, B> host;
  DeviceBuf<T, B> dev;
  Event<B> done;
  // Room for `count` elements (a new pair of copies holds at least `at_least`).  A pair that is too small is replaced: the
  // upload out of the old pinned copy and the work on `st` that may still read the old device copy are waited for first.
  // *fresh: the copies are new (their contents undefined).  A failed call leaves the pair as it was or empty.
  Status begin(size_t count, size_t at_least, typename B::Stream st, T** out, bool* fresh = nullptr) {
    bool is_new = false;
    if (!dev.p || dev.cap < count) {
      if (Status s = done.wait_if_recorded(); !s.ok()) return s;
      done.recorded = false;
      if (Status s = release_group<B>(st, dev, host); !s.ok()) return s;
      const size_t cap = std::max(count, at_least);
      if (Status s = ensure_group(&is_new, want(dev, cap), want(host, cap)); !s.ok()) return s;
      if (Status s = done.ensure(); !s.ok()) {
        (void)dev.reset();
        (void)host.reset();
        return s;
      }
    }
    if (fresh) *fresh = is_new;
    if (Status s = done.wait_if_recorded(); !s.ok()) return s;
    *out = host.p;
    return {};
  }
  Status commit(size_t count, typename B::Stream st) {
    if (int e = B::copy_to_device(dev.p, host.p, sizeof(T) * count, st)) return {e, 0};
    const Status s = done.record(st);
    if (!s.ok()) (void)B::stream_wait(st);             // (the copy is enqueued and nothing could wait for it: drain the stream)
    return s;
  }
  T* device() const { return dev.p; }
};

// The input ring: SLOTS slots of per-trajectory records, used in order.  The caller keeps the buffers -- a pinned and a device one
// of SLOTS slots each; several pairs may share one ring -- and indexes them with the slot take() hands out.  The host may refill a
// pinned slot once the work that read it has run, tracked per GROUP of slots: the group's event is recorded behind the work that
// read its last slot and waited for when the ring comes round to its first slot again.  A call goes take, fill the pinned slot,
// submit, launch, launched.  Staged (`direct` = false): submit copies the slot to the device, which the kernels read, and the slot
// is done; direct: the kernels read the pinned slot itself and the slot is done behind their launch.  A call that fails between
// take and the end leaves its group open with no event behind it: the next trip round waits for the whole stream.
template <class B, int SLOTS, int GROUP> struct InputRing {
  static_assert(SLOTS % GROUP == 0, "whole groups");
  Event<B> ev[SLOTS / GROUP];
  bool open[SLOTS / GROUP] = {};
  int pos = 0;
  Status ensure() {
    for (auto& e : ev)
      if (Status s = e.ensure(); !s.ok()) return s;
    return {};
  }
  // (a failed take leaves the ring where it was: the slot has not been waited for)
  Status take(typename B::Stream st, int* slot) {
    const int s = pos, g = s / GROUP;
    if (s % GROUP == 0) {
      if (open[g]) {                                   // (a failed call left the group without its event)
        if (int e = B::stream_wait(st)) return {e, 0};
      } else if (Status w = ev[g].wait_if_recorded(); !w.ok()) {
        return w;
      }
    }
    pos = (s + 1) % SLOTS;
    open[g] = true;
    *slot = s;
    return {};
  }
  Status submit(int slot, bool direct, void* dev, const void* host, size_t bytes, typename B::Stream st) {
    if (direct) return {};
    if (int e = B::copy_to_device(dev, host, bytes, st)) return {e, 0};
    return done(slot, st);
  }
  Status launched(int slot, bool direct, typename B::Stream st) { return direct ? done(slot, st) : Status{}; }

 private:
  Status done(int slot, typename B::Stream st) {
    if (slot % GROUP != GROUP - 1) return {};
    if (Status s = ev[slot / GROUP].record(st); !s.ok()) return s;
    open[slot / GROUP] = false;
    return {};
  }
};

}  // namespace res
}  // namespace ekf
