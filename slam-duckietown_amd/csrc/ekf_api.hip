// C ABI of libekfslam_hip.so (include/ekfslam_hip.h): host-side orchestration of the HIP kernels.
// No CPU fallback exists: every entry point needs a gfx950 device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "ekf_device.h"
#include "ekf_host_plan.h"
#include "ekf_launch.h"
#include "ekf_resources.h"

using namespace ekf;

static thread_local std::string g_create_error;

// Stream pairs outlive their handles.  A handle drives two HIP streams (its own and the one the look-ahead sends the covariance
// pass to, beside the next cadence's solve).  HIP maps streams onto a few hardware queues as they are created; measured on this
// pool: the second handle of a process -- created after the first one's streams had been destroyed -- ran its pass and the solve
// beside it 10 % slower (N = 8000 x 1: 389 us against 355 us; 355 us again with lookahead = 0: the two streams no longer ran
// side by side), whatever memory it was given (tools/leg_order_probe.py, profiles/r04_dense_operands.txt part 2).  So the pair
// a destroyed handle leaves is parked here, per device, and the next handle on that device takes it over: the mapping the
// first pair got in a fresh process is the one every later handle runs on.  (Streams are idle when parked: free_all
// synchronises them.)
#include <mutex>
struct StreamPair { int device; hipStream_t stream, aux; };
static std::mutex g_pairs_mu;
static std::vector<StreamPair> g_pairs;
static bool take_stream_pair(int device, hipStream_t* stream, hipStream_t* aux) {
  std::lock_guard<std::mutex> lk(g_pairs_mu);
  for (size_t i = 0; i < g_pairs.size(); ++i)
    if (g_pairs[i].device == device) {
      *stream = g_pairs[i].stream;
      *aux = g_pairs[i].aux;
      g_pairs.erase(g_pairs.begin() + (long)i);
      return true;
    }
  return false;
}
static void park_stream_pair(int device, hipStream_t stream, hipStream_t aux) {
  std::lock_guard<std::mutex> lk(g_pairs_mu);
  g_pairs.push_back({device, stream, aux});
}

constexpr int RING = 16;
constexpr int RING_GROUP = 4;             // slots per completion event: an event record between two launches costs the
                                          // stream a barrier packet, ~2 us per online step of a small filter
constexpr int PACK_SMALL_N = 131;        // states up to 64 landmarks are downloaded by k_pack_small (137 KB of pinned memory)

// How the ownership types of ekf_resources.h reach the runtime: the only allocations, frees, event creations and destructions
// of this file (beside ekf_host_alloc / ekf_host_free, the ABI's own).
struct HipBackend {
  using Stream = hipStream_t;
  using Event = hipEvent_t;
  static constexpr unsigned pinned_default = hipHostMallocDefault;
  static int device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static int device_free(void* p) { return hipFree(p); }
  static int pinned_alloc(void** p, size_t bytes, unsigned flag) { return hipHostMalloc(p, bytes, flag); }
  static int pinned_free(void* p) { return hipHostFree(p); }
  static int event_create(Event* e, bool timing) { return timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming); }
  static int event_destroy(Event e) { return hipEventDestroy(e); }
  static int event_record(Event e, Stream st) { return hipEventRecord(e, st); }
  static int event_wait(Event e) { return hipEventSynchronize(e); }
  static int stream_wait(Stream st) { return hipStreamSynchronize(st); }
  static int copy_to_device(void* dst, const void* src, size_t bytes, Stream st) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  }
};
template <class T> using DeviceBuf = res::DeviceBuf<T, HipBackend>;
template <class T> using PinnedBuf = res::PinnedBuf<T, HipBackend>;
template <class T> using StagedUpload = res::StagedUpload<T, HipBackend>;
using Event = res::Event<HipBackend>;
using InputRing = res::InputRing<HipBackend, RING, RING_GROUP>;

struct ekf_handle : ekf::HostPlan {
  DeviceConfig dcfg{};
  hipStream_t stream = nullptr;
  // Every buffer and event below is owned by its member (ekf_resources.h) and released when the handle is deleted (free_all).
  DeviceBuf<double> dP, dV, dW, dscratch;
  DeviceBuf<double> ddacc2[2];    // pending pose-block noise, double-buffered like the mean
  int dcur = 0;
  DeviceBuf<double> dmu2[2];      // the mean is double-buffered: a step reads [cur], writes [cur^1]
  int cur = 0;
  DeviceBuf<int> dn;
  DeviceBuf<unsigned> dflags;
  DeviceBuf<SolveOut> dso;
  DeviceBuf<double> dfac;         // pending factors restricted to the gathered indices (k_solve -> k_panels)
  DeviceBuf<StepIn> d_ring;
  PinnedBuf<StepIn> h_ring;
  InputRing ring;                 // the slots of h_ring / d_ring, h_det / d_det and h_pred / d_pred: one position, one set of events
  DeviceBuf<StepIn> d_stream;
  DeviceBuf<int> dfloor;          // per trajectory floor of the active bound, applied by k_solve (see push_floor)
  DeviceBuf<double> dF, dQ, dTmp; // dense path, allocated on first use (one group)
  DeviceBuf<double> dPlin;        // dense path with P in column panels: its row-major staging copy
  // device-side association (one group, allocated on first use: assoc_init)
  DeviceBuf<int> dtagmap, dneff;
  DeviceBuf<DetIn> d_det;
  PinnedBuf<DetIn> h_det;
  DeviceBuf<StepIn> d_assoc_step;
  DeviceBuf<AssocOut> d_assoc_out;
  AssocConfig acfg{};
  Event t0, t1;
  bool profile = false;
  int profile_stride = 1;         // every how many launches of the pass carry an event pair while profiling ("profile_stride")
  long prof_seen = 0;
  std::vector<Event> prof_pool;
  size_t prof_used = 0;
  // "profile_kernels" = 1: the cadence's other launches carry event pairs too (a diagnostic run: every record costs its stream
  // ~6 us); class of pair i: 0 the covariance pass, 1 the solve launch, 2 the chain / look-ahead gather launch, 3 the panel launch
  int opt_profile_kernels = 0;
  std::vector<int> prof_cls;
  DeviceBuf<unsigned> dqueue;     // work-queue heads of k_flush_rs (zeroed before every launch)
  // k_flush_rs, equal static shares (a few long trajectories): the piece table.  Two copies, used alternately: a rebuilt
  // table is uploaded stream-ordered, without a host synchronisation, while the pass that read the previous one may still be
  // running.
  StagedUpload<int> shares2[2];
  int shares_cur = 0;
  int shares_key[4] = {0, 0, 0, 0};   // (batch, slabs, last strip, workgroups) the current table was built for
  int shares_ok = 0;              // pieces of its longest share (0: no table for this key -- the queue modes are used)
  DeviceBuf<unsigned> dready;     // per trajectory: sequence number of the last solve that completed (k_step_split)
  DeviceBuf<SolveOut> dmbox;      // per trajectory: that solve's header and records, written through (mailbox_publish)
  unsigned step_seq = 0;          // sequence number of the last single-launch step
  // per trajectory: head + per-landmark records of a cadence (allocated on first use).  Two copies, used alternately by
  // consecutive cadences (`run.cpar`): in a chained run the next cadence's solve writes its records while this cadence's panel
  // launch still reads these.  (The cadences' counters, parities and statistics: ekf_host_plan.h, CadRun -- h->run.)
  DeviceBuf<CadOut> dcad2[2];
  // Chained solves (round 6; "chain"): the solves of a run follow one another on the handle's stream -- the next cadence's
  // block comes from this cadence's records (k_chain_cad) -- while panel launch and covariance pass of every cadence run
  // on the second stream.  dprow3: rows 0..2 of every P after a cadence, left by its panel launch (batch x 3 x ld, two copies
  // like dcad2); dgmu: the mean at the next cadence's positions (batch x 128).
  DeviceBuf<double> dprow3[2];
  DeviceBuf<double> dgmu;
  DeviceBuf<double> dxg, dbg;     // the chain launch's gathered rows (batch x 84 x 88 each): written by its gather workgroups
  DeviceBuf<unsigned> dsync;      // device-scope counters of the chained run's hand-overs (ekf_cadence.hip: SYNC_*)
  DeviceBuf<CadPre> dpre[2];      // a cadence's inputs formed one cadence ahead: two copies (run.pre_serial: whose inputs a copy holds)
  Event ev_pass;                  // recorded on the second stream when a chain of cadences ends (join_aux): the only event of the chained order
  int opt_run_end_flush = 0;      // 1 = ekf_stream_run applies what its last cadence left pending, so that the next call starts fused
  // The mirrored column entries of a cadence's panel launch, gathered by extra workgroups of its solve launch and laid down
  // as rows (batch x 83 x ld doubles, allocated on first use; not for banks where that would exceed 1 GiB; "col_gather")
  DeviceBuf<double> dcolbuf;
  // The packed cadences of the ekf_stream_run in flight (ekf_host_plan.h: plan_cadences): one CadPlan per (cadence,
  // trajectory), planned on the host for the whole run and uploaded once, stream-ordered, out of pinned memory.  Two copies,
  // used alternately: the host may plan the next run while the upload of this one has not executed yet.
  RunPlan run_plan;
  StagedUpload<CadPlan> plan2[2];
  int plan_cur = 0;
  // look-ahead (small launches): the solve of the next cadence runs on the handle's stream beside the covariance pass of
  // this one, which goes to a second stream between two events; see ekf_stream_run
  hipStream_t aux = nullptr;
  Event ev_fork, ev_join;
  DeviceBuf<double> dgbuf;        // per trajectory: the next cadence's block, gathered while this one's ranks are pending
  long assoc_fallbacks = 0;       // statistics: windows a binding took through the host association (ekf_debug_note_assoc_fallback)
  long small_launches = 0;        // statistics: launches of the small-state path (k_small_stream)
  long fused_fetches = 0;         // statistics: ekf_step_fetch calls answered by the step's own launch
  long dense_packs = 0;           // statistics: large downloads written by k_pack_dense (pinned destination)
  int opt_pack_dense = 1;
  int fetch_b = -1;               // ekf_step_fetch: the trajectory whose state the next small-state launch leaves in h_pack
  bool fetched = false;
  unsigned long long fetch_seq = 0;   // ... and the sequence number that launch releases behind it (polled by the host)
  int opt_fetch_spin = 1;
  int opt_fetch_verify = 1;       // 1 (default) = ekf_step_fetch checks the payload's XOR checksum before it trusts a polled hand-over (~1 us of the 10 - 15 us the polling saves); 0 = the trailer's second sequence number only
  long fetch_retries = 0;         // statistics: hand-overs whose integrity trailer did not match (answered after a stream sync)
  int last_kernel = -1, last_nkt = 0, last_streaming = 0;   // what the last covariance pass launched
  int last_wv = 0;                // ... and whether it formed its W fragments from V ("w_from_v")
  int last_shares = 0;            // ... and whether it ran on equal static shares (k_flush_rs, a few long trajectories)
  std::vector<unsigned> flags_host;
  PinnedBuf<unsigned> h_flags;    // pinned: the sticky flags are read back with a stream-ordered copy
  PinnedBuf<double> h_pack{hipHostMallocCoherent};   // pinned, coherent: where k_pack_small leaves a small state (n x n covariance, mean, flags)
  // The read-only queries' staging buffer: a query's inputs, then its destinations that are not pinned (StagingPlan).  Every
  // query synchronises the stream before it returns, so the next one finds the buffer free.
  DeviceBuf<double> dquery;
  std::vector<int> joint_sel;     // ekf_download_joint: the selection as the host sorted it (plan_joint_query)
  std::vector<std::pair<int, int>> joint_order;   // ... scratch of the sort (handle-owned: no allocation per query)
  // ekf_factor (allocated on first use, released by ekf_factor_release): the workspace of the Cholesky factors, each factored
  // trajectory's status words {info, n, nblk, 0} and log-determinant; `factor` is what the host remembers of the snapshot
  DeviceBuf<double> dfactor, dflog;
  DeviceBuf<int> dfstat;
  ekf::FactorHeld factor;
  std::vector<double> factor_log;
  std::vector<int> factor_stat;   // ... and the status words as they come back
  // The innovation log (ekf_log_innovations; empty: off): a ring of innov_cap step rows, innov_steps steps logged so far.
  // While an entry point enqueues a logged step, lg_slot is the ring row of its next launch (-1: that launch is not logged) and
  // lg_jbase the position of its first landmark; ekf_stream_run logs stream step t in row (lg_tslot + t) % innov_cap.
  DeviceBuf<InnovRec> dinnov;
  DeviceBuf<int> dinnov_m;
  int innov_cap = 0;
  long long innov_steps = 0;
  long lg_slot = -1, lg_tslot = -1;
  int lg_jbase = 0;
  // The pose log (ekf_log_poses; empty: off): a ring of pose_cap step rows (batch x POSE_ROW doubles each), pose_steps steps
  // logged so far; a counter of its own -- a lone prediction is a row here and none in the innovation log.  While an entry
  // point enqueues a step, pl_slot is its ring row (-1: nothing is logged); ekf_stream_run logs stream step t in row
  // (pl_tslot + t) % pose_cap.
  DeviceBuf<double> dpose;
  int pose_cap = 0;
  long long pose_steps = 0;
  long pl_slot = -1, pl_tslot = -1;
  // The NIS gate (ekf_set_nis_gate): per-trajectory rejection counters, allocated when the gate is first switched on.  While
  // the gate is on dcfg.gate_rej points at them and dcfg.nis_gate holds the threshold (kernel arguments: every launch
  // enqueued after the call sees the new value).
  DeviceBuf<unsigned long long> dgate;
  // Per-trajectory noise constants (ekf_set_noise), allocated on the first call: noise_ms / noise_qs are the sigmas in effect
  // for work enqueued next (ekf_get_noise reads them), `noise` the table of their rows.  dcfg.noise points at its device copy
  // while some row differs from the handle's constants, nullptr otherwise (the kernels without the table).  The upload goes
  // through its pinned copy, which is written again only once the event recorded behind the previous copy has completed.
  std::vector<double> noise_ms, noise_qs;
  StagedUpload<double> noise;
  // Set when an enqueueing call failed half way (e.g. a launch of the look-ahead failed after the next cadence's solve had
  // already run): the device state of every trajectory is undefined until it is uploaded again; see check_internal
  std::vector<unsigned char> host_bad;
  // ekf_remove_landmarks (allocated on first use): the launch's index tables (src then dst, ld ints each), the row
  // announcements of k_remove (batch x ld words) and the sequence number the last launch announced with.  stream_stale: the
  // uploaded stream was validated against sizes a removal has changed since (ekf_stream_run refuses it)
  DeviceBuf<int> drm_tab;
  DeviceBuf<unsigned> drm_flag;
  unsigned rm_seq = 0;
  bool stream_stale = false;
  // ekf_copy_trajectories (allocated on first use, in the DESTINATION handle): the launch's table of groups (plan_copy)
  DeviceBuf<int> dcp_tab;
  // ekf_join_maps (allocated on first use, in the DESTINATION handle): the launch's table of pairs (plan_join) and the snapshot
  // of every destination's pose, its 3 x 3 block and its three pose rows as they stood before the join (join_snap_doubles per pair)
  DeviceBuf<int> djn_tab;
  DeviceBuf<double> djn_snap;
  // ekf_transform (allocated on first use): the launch's table (plan_transform) and its frames -- the plan's heads, then the means
  // of the call's range as they stood before the call (transform_frame_doubles per trajectory)
  DeviceBuf<int> dtf_tab;
  DeviceBuf<double> dtf_frame;
  // ekf_update_direct / ekf_update_linear (allocated on first use, grown to the larger need: the two calls never overlap, each
  // ends in a synchronise): the table of the front's launch for the bank (ekf_host_plan.h: FrontTable -- the plan's ints, the
  // measurements, the results NIS and applied), its host sides, and each call's plan
  DeviceBuf<double> dfront;
  std::vector<int> front_ints;
  std::vector<double> front_dbls, front_out;
  ekf::DirectPlan direct_plan;
  ekf::LinearPlan linear_plan;
  // ekf_predict_linear (allocated on first use): the input ring of k_predict_pose's records, RING slots of batch records used
  // in the order of h_ring / d_ring and under the same events (`ring`), and the call's plan
  DeviceBuf<PredictIn> d_pred;
  PinnedBuf<PredictIn> h_pred;
  ekf::PredictPlan predict_plan;
  // ekf_localize_* (allocated on first use): what k_loc_solve hands to k_loc_rows, one record per trajectory; consecutive steps
  // reuse it in stream order
  DeviceBuf<LocRec> dloc;
  // ekf_localize_detections (allocated on first use): per trajectory, the tags of its last localisation window that its map does
  // not hold (k_loc_associate; ekf_download_unmatched).  A property of the slot: a copy or a join leaves it as it is
  DeviceBuf<LocUnmatched> d_unmatched;
  std::string err;
};

static int fail(ekf_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

static int bad_arg(ekf_handle* h, const char* fn, const std::string& why) { return fail(h, EKF_ERR_ARG, std::string(fn) + ": " + why); }

static int flush_pending(ekf_handle* h);
static int flush_pending(ekf_handle* h, hipStream_t st, const CadOut* wv = nullptr);
static int materialize(ekf_handle* h, int b);

#define HIP_TRY(h, expr)                                                                   \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(h, EKF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

// What an ownership operation (ekf_resources.h) reports, as this file's error: `what` names the buffer or group.
static int res_fail(ekf_handle* h, const char* what, const res::Status& s) {
  return fail(h, EKF_ERR_HIP, std::string(what) + (s.bytes ? ": allocation of " + std::to_string(s.bytes) + " bytes" : std::string()) +
                                  ": " + hipGetErrorString((hipError_t)s.err));
}
#define RES_TRY(h, what, expr)                                                             \
  do {                                                                                     \
    const res::Status s_ = (expr);                                                         \
    if (!s_.ok()) return res_fail(h, what, s_);                                            \
  } while (0)

// The device's view of a pinned host allocation (ekf_host_alloc), which a kernel can write in place; nullptr for anything else.
static void* device_view(void* p) {
  hipPointerAttribute_t attr{};
  if (p && hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost) return attr.devicePointer;
  (void)hipGetLastError();                             // (an ordinary pointer is "invalid value" to the query)
  return nullptr;
}

// Copies between a host matrix (row-major, `host_pitch` doubles per row) and the block [r0, r0 + rows) x [c0, c0 + cols) of
// trajectory b's covariance in its device layout (ekf_device.h: row-major up to ld = 4096, column panels of 4096 doubles
// beyond): one 2-D copy per column panel the block touches.  `other` = nullptr: the host side; else a device matrix in
// plain row-major (the dense product's staging), copied device to device.
static hipError_t copy_cov(ekf_handle* h, int b, double* host, int host_pitch, int r0, int c0, int rows, int cols, bool to_device,
                           bool device_to_device = false) {
  for (int p = c0 / PPW; p <= (c0 + cols - 1) / PPW; ++p) {
    const int cs = std::max(c0, p * PPW), ce = std::min(c0 + cols, (p + 1) * PPW);
    double* dev = h->dP.p + (size_t)b * h->pstride + p_index(h->ld, r0, cs);
    double* hst = host + (cs - c0);
    const size_t dpitch = sizeof(double) * (size_t)p_lds(h->ld), hpitch = sizeof(double) * (size_t)host_pitch;
    const size_t width = sizeof(double) * (size_t)(ce - cs);
    const hipMemcpyKind kind = device_to_device ? hipMemcpyDeviceToDevice : (to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
    const hipError_t e = to_device ? hipMemcpy2DAsync(dev, dpitch, hst, hpitch, width, (size_t)rows, kind, h->stream)
                                   : hipMemcpy2DAsync(hst, hpitch, dev, dpitch, width, (size_t)rows, kind, h->stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" int ekf_config_default(ekf_config* cfg) {
  if (!cfg) return EKF_ERR_ARG;
  cfg->motion_sigma = 0.1;
  cfg->meas_sigma = 0.7;
  cfg->arc_threshold = 1e-2;
  cfg->landmark_init_var = 10000.0;
  cfg->enable_measurement_model = 1;
  cfg->enable_circular_interpolation = 1;
  cfg->disable_motion_model = 0;
  cfg->reserved = 0;
  return EKF_OK;
}

extern "C" int ekf_device_count(int* count) {
  if (!count) return EKF_ERR_ARG;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *count = c;
  return EKF_OK;
}

// Pinned host memory for the arrays a binding hands to its caller (see include/ekfslam_hip.h).
extern "C" void* ekf_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
extern "C" void ekf_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

extern "C" const char* ekf_last_error(ekf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// The handle's members release what they own (ekf_resources.h) when it is deleted: with its device selected and both streams idle.
static void free_all(ekf_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->aux) (void)hipStreamSynchronize(h->aux);
  const int device = h->device;
  const hipStream_t stream = h->stream, aux = h->aux;
  delete h;
  if (stream && aux) {
    park_stream_pair(device, stream, aux);             // (see g_pairs: the next handle on this device takes the pair over)
  } else {
    if (aux) (void)hipStreamDestroy(aux);
    if (stream) (void)hipStreamDestroy(stream);
  }
}

extern "C" int ekf_create(int device, int n_max, int batch, const ekf_config* cfg, ekf_handle** out) {
  if (!out) return fail(nullptr, EKF_ERR_ARG, "ekf_create: out is NULL");
  *out = nullptr;
  if (n_max < 3 || (n_max & 1) == 0) return fail(nullptr, EKF_ERR_ARG, "ekf_create: n_max must be 3 + 2*N");
  if (batch < 1) return fail(nullptr, EKF_ERR_ARG, "ekf_create: batch must be >= 1");
  // The kernels address one trajectory's covariance with unsigned 32-bit byte offsets (buffer instructions: k_flush_rs,
  // k_solve's staging, k_gemm_f64's resources): what is allocated for it must stay below 4 GiB.  Checked before the device is
  // looked for, so that the limit can be tested without one.
  {
    const int rows = (n_max + 63) / 64 * 64;             // (= ld beyond 4096, where the covariance is kept in column panels)
    if (n_max > EKF_N_MAX_LIMIT || (unsigned long long)p_alloc(rows, rows) * 8ull >= (1ull << 32))
      return fail(nullptr, EKF_ERR_ARG,
                  "ekf_create: n_max = " + std::to_string(n_max) + " exceeds EKF_N_MAX_LIMIT = " +
                      std::to_string(EKF_N_MAX_LIMIT) + " (one covariance must stay below 4 GiB: 32-bit byte offsets)");
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, EKF_ERR_HIP, std::string("ekf_create: no HIP device (") + hipGetErrorString(e) +
                                          "); this library has no CPU fallback");
  if (device < 0 || device >= count) return fail(nullptr, EKF_ERR_ARG, "ekf_create: device index out of range");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
    return fail(nullptr, EKF_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, EKF_ERR_HIP, std::string("ekf_create: device is ") + prop.gcnArchName +
                                          ", kernels are built for gfx950 only");
  ekf_handle* h = new ekf_handle();
  h->device = device;
  h->cu_count = prop.multiProcessorCount;
  h->n_max = n_max;
  // Row stride of P: a multiple of 64 doubles (every 64-column strip of the pass lies inside the row, 512-B aligned)
  // and, up to 4096, a power of two: with rows exactly 32 KB (or 16, 8 ... KB) apart the sixteen 512-byte row
  // segments of a tile fall into the same DRAM pages instead of sixteen different ones -- measured on the pass at
  // N=2000 x 32: 775 us with ld = 4032, 729 us with ld = 4096; N=1500: 767 -> 696 us; larger strides (ld = 8192) are
  // slower than the plain round-up, so beyond 4096 the stride is n_max rounded up to 64 (profiles/r02_ld_sweep.txt).
  h->rows = (n_max + 63) / 64 * 64;                    // rows allocated per trajectory
  h->ld = h->rows;
  if (n_max <= 4096) {
    int p2 = 64;
    while (p2 < n_max) p2 *= 2;
    h->ld = p2;
  }
  h->batch = batch;
  h->pstride = p_alloc(h->rows, h->ld);                // (column panels of 4096 doubles beyond ld = 4096: ekf_device.h)
  if (cfg) h->cfg = *cfg; else ekf_config_default(&h->cfg);
  if (const char* e = std::getenv("EKFSLAM_HIP_SMALL_STATE")) h->opt_small_state = std::atoi(e) != 0;   // (tests pin the general kernels at small sizes)
  if (const char* e = std::getenv("EKFSLAM_HIP_FETCH_SPIN")) h->opt_fetch_spin = std::atoi(e) != 0;
  const double s = h->cfg.motion_sigma, q = h->cfg.meas_sigma;
  h->dcfg.rd[0] = s * s;                        // src/replay_no_ros.py:421
  h->dcfg.rd[1] = s * s;
  h->dcfg.rd[2] = (s / 2) * (s / 2);
  h->dcfg.qd[0] = q * q;                        // :438
  h->dcfg.qd[1] = q * q;
  h->dcfg.arc_threshold = h->cfg.arc_threshold;
  h->dcfg.enable_measurement_model = h->cfg.enable_measurement_model;
  h->dcfg.enable_circular_interpolation = h->cfg.enable_circular_interpolation;
  h->dcfg.disable_motion_model = h->cfg.disable_motion_model;
  h->acfg.gate2 = 1.5 * 1.5;                      // src/replay_no_ros.py:289
  h->acfg.init_var = h->cfg.landmark_init_var;
  h->acfg.n_ignore = 0;
  h->acfg.active_bound = 1;
  h->n.assign(batch, 3);
  h->neff.assign(batch, 3);
  h->neff_enq.assign(batch, 3);
  h->floor_host.assign(batch, 3);
  h->host_bad.assign(batch, 0);

#define CREATE_TRY(expr)                                                                  \
  do {                                                                                    \
    hipError_t e2_ = (expr);                                                              \
    if (e2_ != hipSuccess) {                                                              \
      g_create_error = std::string(#expr) + ": " + hipGetErrorString(e2_);                \
      free_all(h);                                                                        \
      return EKF_ERR_HIP;                                                                 \
    }                                                                                     \
  } while (0)
#define CREATE_RES(what, expr)                                                            \
  do {                                                                                    \
    const res::Status s_ = (expr);                                                        \
    if (!s_.ok()) {                                                                       \
      (void)res_fail(nullptr, "ekf_create: " what, s_);                                   \
      free_all(h);                                                                        \
      return EKF_ERR_HIP;                                                                 \
    }                                                                                     \
  } while (0)
  CREATE_TRY(hipSetDevice(device));
  if (!take_stream_pair(device, &h->stream, &h->aux)) {
    CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    // The second stream gets the LOWEST priority: the runtime multiplexes streams onto a few hardware queues per priority level,
    // so a priority of its own keeps it off the hardware queue of the handle's own stream however many streams the process has
    // created (two streams on one queue run one behind the other: the chained order stays correct -- every wait is for an
    // earlier-enqueued launch -- but nothing overlaps); and what runs there (panel launches, covariance passes) is the work
    // that may wait.  No measurable effect on a fresh process (profiles/r06_chained_solves.txt).
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    if (const char* e = std::getenv("EKFSLAM_HIP_AUX_PRIORITY")) least = std::atoi(e);
    if (hipStreamCreateWithPriority(&h->aux, hipStreamNonBlocking, least) != hipSuccess) {
      (void)hipGetLastError();
      CREATE_TRY(hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking));
    }
  }
  CREATE_RES("ev_fork", h->ev_fork.ensure());
  CREATE_RES("ev_join", h->ev_join.ensure());
  CREATE_RES("ev_pass", h->ev_pass.ensure());
  const size_t ldz = (size_t)h->ld, B = (size_t)batch;
  CREATE_RES("dP", h->dP.ensure((size_t)h->pstride * B));
  CREATE_RES("dmu2[0]", h->dmu2[0].ensure(ldz * B));
  CREATE_RES("dmu2[1]", h->dmu2[1].ensure(ldz * B));
  CREATE_RES("dV", h->dV.ensure(ldz * KTOT * B));
  CREATE_RES("dW", h->dW.ensure(ldz * KTOT * B));
  CREATE_RES("ddacc2[0]", h->ddacc2[0].ensure(4 * B));
  CREATE_RES("ddacc2[1]", h->ddacc2[1].ensure(4 * B));
  CREATE_RES("dscratch", h->dscratch.ensure(ldz * 2));
  CREATE_RES("dn", h->dn.ensure(B));
  CREATE_RES("dflags", h->dflags.ensure(B));
  CREATE_RES("dfloor", h->dfloor.ensure(B));
  CREATE_RES("dqueue", h->dqueue.ensure((size_t)flush_rs_queue_words()));
  CREATE_RES("dready", h->dready.ensure(B));
  CREATE_RES("dmbox", h->dmbox.ensure(B));
  CREATE_TRY(hipMemsetAsync(h->dmbox.p, 0, sizeof(SolveOut) * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dready.p, 0, sizeof(unsigned) * batch, h->stream));
  CREATE_RES("dso", h->dso.ensure(B));
  CREATE_RES("dfac", h->dfac.ensure((size_t)FACS * B));
  CREATE_RES("d_ring", h->d_ring.ensure(B * RING));
  CREATE_RES("h_ring", h->h_ring.ensure(B * RING));
  CREATE_RES("h_flags", h->h_flags.ensure(B));
  CREATE_RES("the input ring's events", h->ring.ensure());
  CREATE_RES("t0", h->t0.ensure(true));
  CREATE_RES("t1", h->t1.ensure(true));
  CREATE_TRY(hipMemsetAsync(h->dP.p, 0, sizeof(double) * (size_t)h->pstride * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dmu2[0].p, 0, sizeof(double) * ldz * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dmu2[1].p, 0, sizeof(double) * ldz * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dV.p, 0, sizeof(double) * ldz * KTOT * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dW.p, 0, sizeof(double) * ldz * KTOT * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->ddacc2[0].p, 0, sizeof(double) * 4 * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->ddacc2[1].p, 0, sizeof(double) * 4 * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dflags.p, 0, sizeof(unsigned) * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dso.p, 0, sizeof(SolveOut) * batch, h->stream));
  CREATE_TRY(hipMemsetAsync(h->dfac.p, 0, sizeof(double) * FACS * batch, h->stream));
  // reference initial state (src/replay_no_ros.py:69-70): mu = 0, P = MOTION_MODEL_VARIANCE * I3
  {
    std::vector<double> p3(3 * 3, 0.0);
    p3[0] = p3[4] = p3[8] = h->cfg.motion_sigma;
    for (int b = 0; b < batch; ++b)
      CREATE_TRY(copy_cov(h, b, p3.data(), 3, 0, 0, 3, 3, true));
    CREATE_TRY(hipMemcpyAsync(h->dn.p, h->n.data(), sizeof(int) * batch, hipMemcpyHostToDevice, h->stream));
    CREATE_TRY(hipMemcpyAsync(h->dfloor.p, h->floor_host.data(), sizeof(int) * batch, hipMemcpyHostToDevice, h->stream));
    CREATE_TRY(hipStreamSynchronize(h->stream));
  }
#undef CREATE_TRY
#undef CREATE_RES
  *out = h;
  return EKF_OK;
}

extern "C" int ekf_destroy(ekf_handle* h) {
  if (!h) return EKF_ERR_ARG;
  free_all(h);
  return EKF_OK;
}

// After a device-side association the state may have grown on the device: read the sizes back.
static int refresh_sizes(ekf_handle* h) {
  if (!h->sizes_dirty) return EKF_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(h->n.data(), h->dn.p, sizeof(int) * h->batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->neff.data(), h->dneff.p, sizeof(int) * h->batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->neff_enq = h->neff;
  h->sizes_dirty = false;
  return EKF_OK;
}

static int check_b(ekf_handle* h, int b, const char* fn) {
  if (!h) return EKF_ERR_ARG;
  if (int rc = refresh_sizes(h)) return rc;
  if (b < 0 || b >= h->batch) return fail(h, EKF_ERR_ARG, std::string(fn) + ": trajectory index out of range");
  return EKF_OK;
}

// A bounded wait of a single-launch step that ran into its limit leaves EKF_FLAG_INTERNAL on the trajectory: the
// timed-out workgroups wrote nothing while others of the same step may have, so the trajectory's state is UNDEFINED from
// there on, until it is uploaded again (ekf_upload_state* clears the flag).  The same holds -- for every trajectory of
// the handle -- after an enqueueing call failed half way (host_bad).  Every call that hands results to the host reports
// it: EKF_ERR_STATE.  b < 0: any trajectory.  Synchronises the handle's stream (the flags come back with a stream-ordered
// copy into pinned memory, on that stream).
static int check_internal(ekf_handle* h, int b, const char* fn) {
  HIP_TRY(h, hipMemcpyAsync(h->h_flags.p, h->dflags.p, sizeof(unsigned) * h->batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int t = (b < 0 ? 0 : b); t < (b < 0 ? h->batch : b + 1); ++t) {
    if (h->host_bad[t])
      return fail(h, EKF_ERR_STATE,
                  std::string(fn) + ": an earlier call on this handle failed after part of its work had been enqueued; the "
                      "state of trajectory " + std::to_string(t) + " is undefined: upload it again (ekf_upload_state / "
                      "ekf_upload_state_diag)");
    if (h->h_flags.p[t] & EKF_FLAG_INTERNAL)
      return fail(h, EKF_ERR_STATE,
                  std::string(fn) + ": trajectory " + std::to_string(t) +
                      " carries EKF_FLAG_INTERNAL (a bounded wait inside a single-launch step timed out; the state is "
                      "undefined): upload the state again (ekf_upload_state / ekf_upload_state_diag) "
                      "and consider ekf_set_option(\"fused_step\", 0)");
  }
  return EKF_OK;
}
// (an upload replaces mean and covariance of trajectory b entirely: the trajectory is good again)
static int clear_internal(ekf_handle* h, int b) {
  HIP_TRY(h, hipMemcpyAsync(h->h_flags.p, h->dflags.p + b, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  unsigned f = h->h_flags.p[0];
  if (f & EKF_FLAG_INTERNAL) {
    f &= ~EKF_FLAG_INTERNAL;
    HIP_TRY(h, hipMemcpy(h->dflags.p + b, &f, sizeof(unsigned), hipMemcpyHostToDevice));
  }
  h->host_bad[b] = 0;
  return EKF_OK;
}
// Stepping calls refuse a handle whose state is undefined after a half-enqueued failure (no synchronisation).
static int check_host_bad(ekf_handle* h, const char* fn) {
  for (int t = 0; t < h->batch; ++t)
    if (h->host_bad[t])
      return fail(h, EKF_ERR_STATE, std::string(fn) + ": an earlier call on this handle failed after part of its work had "
                                        "been enqueued; upload every trajectory again before stepping");
  return EKF_OK;
}

static int check_range(ekf_handle* h, const char* fn, int b0, int count) {
  if (!h) return EKF_ERR_ARG;
  return bank_range_ok(h, b0, count) ? EKF_OK : bad_arg(h, fn, BANK_RANGE_WHY);
}

// ---- the read-only queries (ekf_download_marginals, ekf_associate, ekf_download_joint) ----
// Each reads the filter as the covariance pass would leave it, without running it (PendingView), and writes only its
// destinations -- pinned ones in place, the others through the handle's staging buffer and one copy each (StagingPlan): nothing
// of the handle's scheduling state changes.  A query is query_begin, q.add per destination, query_stage, its uploads and
// launch, query_end.
struct Query {
  StagingPlan plan;
  void *host[STAGE_DSTS], *dev[STAGE_DSTS];            // dev: where the kernels write destination i (nullptr: absent or empty)
  void add(void* p, size_t words) {
    host[plan.ndst] = p;
    dev[plan.ndst] = p && words ? device_view(p) : nullptr;
    plan.add(p != nullptr, words, dev[plan.ndst] != nullptr);
  }
  template <class T> T* out(int i) const { return static_cast<T*>(dev[i]); }
};
// The checks in the order a caller sees them: the handle (which refreshes the sizes a device-side association grew), `early`
// (what is wrong with an argument that the entry point has always tested first; nullptr: nothing), the range, the entry
// point's own argument checks (`site`: returns its failure), then the trajectories an earlier failure left undefined.
template <class SiteChecks>
static int query_begin(ekf_handle* h, const char* fn, int b0, int count, const char* early, SiteChecks site) {
  if (int rc = check_b(h, 0, fn)) return rc;
  if (early) return bad_arg(h, fn, early);
  if (int rc = check_range(h, fn, b0, count)) return rc;
  if (int rc = site()) return rc;
  for (int b = b0; b < b0 + count; ++b)
    if (h->host_bad[b]) return check_internal(h, b, fn);
  HIP_TRY(h, hipSetDevice(h->device));
  return EKF_OK;
}
// Room for the query's inputs and staged destinations; the inputs start at h->dquery.p.
static int query_stage(ekf_handle* h, Query& q) {
  RES_TRY(h, "the queries' staging buffer", h->dquery.reserve(plan_staging(q.plan), 0, h->stream));
  for (int i = 0; i < q.plan.ndst; ++i)
    if (q.plan.dst[i].staged) q.dev[i] = h->dquery.p + q.plan.dst[i].at;
  return EKF_OK;
}
// Behind the launch: the staged destinations, then the flags (check_internal's copy), and the query's one synchronisation.
static int query_end(ekf_handle* h, const char* fn, int b0, int count, const Query& q) {
  HIP_TRY(h, hipGetLastError());
  for (int i = 0; i < q.plan.ndst; ++i)
    if (q.plan.dst[i].staged)
      HIP_TRY(h, hipMemcpyAsync(q.host[i], q.dev[i], sizeof(double) * q.plan.dst[i].words, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->h_flags.p, h->dflags.p, sizeof(unsigned) * h->batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int b = b0; b < b0 + count; ++b)
    if (h->h_flags.p[b] & EKF_FLAG_INTERNAL) return check_internal(h, b, fn);
  return EKF_OK;
}
static PendingView pending_view(const ekf_handle* h, int b0, int count) {
  return PendingView{h->dP.p, h->dV.p, h->dW.p, h->ddacc2[h->dcur].p, h->dmu2[h->cur].p, h->dn.p, h->dso.p, h->ld, h->pstride, b0, count,
                     pending_kb(h)};
}

static BankView bank_view(const ekf_handle* h) { return BankView{h->dP.p, h->dV.p, h->dW.p, h->dn.p, h->dso.p, h->dflags.p, h->dqueue.p, h->ld, h->pstride, h->batch}; }
// The halves of the double-buffered arrays a step's or a cadence's launches read and write; the enqueueing function flips cur,
// dcur (and cpar) behind the step.  dmu2[cur] is the mean the step reads -- of cadence c: its landmark entries are the mean
// before the cadence --, dmu2[cur ^ 1] the one it writes (the one cadence c's solve leaves the pose in); ddacc2[dcur] the
// pending pose noise, ddacc2[dcur ^ 1] what the step leaves pending; dcad2[cpar] cadence c's records; dprow3[cpar ^ 1] the pose
// rows BEFORE it (taken from P_base by launch_snap_pose in front of a chained run's first cadence), dprow3[cpar] where its panel
// launch leaves them.  CAD_NEXT: the cadence after the handle's current one -- every parity the other way round --, for the
// solve enqueue_cadence runs ahead (chained: before it flips the handle; look-ahead: behind the flip, the same copies).
static StepBufs step_bufs(const ekf_handle* h, CadWhich which = CAD_THIS) {
  const int cur = h->cur ^ which, dcur = h->dcur ^ which, cpar = h->run.cpar ^ which;
  return StepBufs{h->dmu2[cur].p, h->dmu2[cur ^ 1].p, h->ddacc2[dcur].p, h->ddacc2[dcur ^ 1].p, h->dcad2[cpar].p, h->dprow3[cpar ^ 1].p,
                  h->dprow3[cpar].p};
}
// Where a launch logs: ring row `slot` of the innovation log (positions from jbase on) and of the pose log.
static InnovLog innov_log(const ekf_handle* h, long slot, int jbase) { return InnovLog{h->dinnov.p, h->dinnov_m.p, slot, h->innov_cap, jbase}; }
static PoseLog pose_log(const ekf_handle* h, long slot) { return PoseLog{h->dpose.p, slot, h->pose_cap}; }
// The largest state of the bank: what sizes a launch's grid.  `device_grown` (the per-step paths, which ekf_step_detections
// runs without reading the sizes back): while sizes_dirty only n_max bounds the states.  ekf_stream_run refreshes the sizes
// before it plans its cadences from h->n, so its launches pass false and read h->n whatever the flag says.
static int bank_n_hi(const ekf_handle* h, bool device_grown) {
  return device_grown && h->sizes_dirty ? h->n_max : *std::max_element(h->n.begin(), h->n.end());
}

static int set_size(ekf_handle* h, int b, int n) {
  h->n[b] = n;
  HIP_TRY(h, hipMemcpyAsync(h->dn.p + b, &h->n[b], sizeof(int), hipMemcpyHostToDevice, h->stream));
  return EKF_OK;
}

// The active bound a step record carries (StepIn.neff) comes from the observations the host saw when the record was
// made.  k_solve raises it to this per-trajectory floor = the bound of the state when the enqueueing call starts
// (or n where the shortcut is switched off), so that a stream uploaded before the state changed -- a dense
// upload, ekf_predict_dense, other steps, a replay of the same stream -- still covers everything correlated.
// exact: the floor must equal the current bound (streams); otherwise it only must not exceed it (single steps
// carry the current bound themselves).
static int push_floor(ekf_handle* h, bool exact) {
  if (h->sizes_dirty) return EKF_OK;                   // device-side association keeps the bound on the device
  bool need = false;
  for (int b = 0; b < h->batch; ++b) {
    const int want = h->opt_active_bound ? h->neff[b] : h->n[b];
    if ((exact || !h->opt_active_bound) ? h->floor_host[b] != want : h->floor_host[b] > want) need = true;
  }
  if (!need) return EKF_OK;
  for (int b = 0; b < h->batch; ++b) h->floor_host[b] = h->opt_active_bound ? h->neff[b] : h->n[b];
  HIP_TRY(h, hipMemcpyAsync(h->dfloor.p, h->floor_host.data(), sizeof(int) * h->batch, hipMemcpyHostToDevice, h->stream));
  return EKF_OK;
}

extern "C" int ekf_upload_state(ekf_handle* h, int b, const double* mu, const double* P, int n) {
  if (int rc = check_b(h, b, "ekf_upload_state")) return rc;
  if (!mu || !P) return fail(h, EKF_ERR_ARG, "ekf_upload_state: NULL array");
  if (n < 3 || (n & 1) == 0 || n > h->n_max) return fail(h, EKF_ERR_ARG, "ekf_upload_state: n must be 3+2N and <= n_max");
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = flush_pending(h)) return rc;
  if (int rc = clear_internal(h, b)) return rc;
  // the upper triangle is what the device keeps (and all it ever reads): blocks of rows, each from its first diagonal
  // column on -- 56 % of the matrix at n = 4003 (1.3 instead of 2.3 ms over PCIe)
  constexpr int UP_ROWS = 512;
  for (int r0 = 0; r0 < n; r0 += UP_ROWS)
    HIP_TRY(h, copy_cov(h, b, const_cast<double*>(P) + (size_t)r0 * n + r0, n, r0, r0, std::min(UP_ROWS, n - r0), n - r0, true));
  HIP_TRY(h, hipMemcpyAsync(h->dmu2[h->cur].p + (size_t)b * h->ld, mu, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  if (int rc = set_size(h, b, n)) return rc;
  h->neff[b] = n;                                      // arbitrary dense covariance: everything is active
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

extern "C" int ekf_upload_state_diag(ekf_handle* h, int b, const double* mu, const double* diagP, int n) {
  if (int rc = check_b(h, b, "ekf_upload_state_diag")) return rc;
  if (!mu || !diagP) return fail(h, EKF_ERR_ARG, "ekf_upload_state_diag: NULL array");
  if (n < 3 || (n & 1) == 0 || n > h->n_max) return fail(h, EKF_ERR_ARG, "ekf_upload_state_diag: n must be 3+2N and <= n_max");
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = flush_pending(h)) return rc;
  if (int rc = clear_internal(h, b)) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->dscratch.p, diagP, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  launch_fill_diag(h->stream, h->dP.p + (size_t)b * h->pstride, h->ld, n, h->dscratch.p);
  HIP_TRY(h, hipGetLastError());
  h->neff[b] = 3;                                      // diagonal covariance: nothing is correlated yet
  HIP_TRY(h, hipMemcpyAsync(h->dmu2[h->cur].p + (size_t)b * h->ld, mu, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  if (int rc = set_size(h, b, n)) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

// The pinned buffer small states come back through (k_pack_small, k_small_stream's host_out): n x n covariance, mean, flags
// word; behind them the integrity trailer of ekf_step_fetch -- sequence number, XOR checksum -- and, at a fixed place at the
// end, the sequence word the host polls.
constexpr size_t PACK_WORDS = (size_t)PACK_SMALL_N * PACK_SMALL_N + PACK_SMALL_N + 4;
static int pack_buffer(ekf_handle* h) {
  if (h->h_pack.p) return EKF_OK;
  RES_TRY(h, "the small-state download buffer", h->h_pack.ensure(PACK_WORDS));
  std::memset(h->h_pack.p, 0, sizeof(double) * PACK_WORDS);
  return EKF_OK;
}

// The step kernels keep only the upper triangle of P_base current.  Before the host (or the dense product)
// looks at trajectory b: apply the pending ranks, then mirror the upper triangle into the lower one.
static int materialize(ekf_handle* h, int b) {
  if (int rc = flush_pending(h)) return rc;
  if (h->sizes_dirty)
    if (int rc = refresh_sizes(h)) return rc;
  launch_mirror(h->stream, h->dP.p + (size_t)b * h->pstride, h->dn.p + b, h->ld, h->pstride, 1, h->n[b]);
  HIP_TRY(h, hipGetLastError());
  return EKF_OK;
}

extern "C" int ekf_download_state(ekf_handle* h, int b, double* mu, double* P, int n) {
  if (int rc = check_b(h, b, "ekf_download_state")) return rc;
  if (n != h->n[b]) return fail(h, EKF_ERR_ARG, "ekf_download_state: n does not match the state size");
  HIP_TRY(h, hipSetDevice(h->device));
  if (P && mu && n <= PACK_SMALL_N) {
    // a small state: flush, then ONE kernel writes covariance (mirrored from the stored triangle), mean and flags into
    // pinned host memory; one synchronisation for everything (see k_pack_small)
    if (h->host_bad[b]) return check_internal(h, b, "ekf_download_state");
    if (int rc = flush_pending(h)) return rc;
    if (int rc = pack_buffer(h)) return rc;
    launch_pack_small(h->stream, h->dP.p + (size_t)b * h->pstride, h->dmu2[h->cur].p + (size_t)b * h->ld, h->dflags.p + b, h->ld, n, h->h_pack.p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((unsigned)h->h_pack.p[(size_t)n * n + n] & EKF_FLAG_INTERNAL) return check_internal(h, b, "ekf_download_state");
    std::memcpy(P, h->h_pack.p, sizeof(double) * (size_t)n * n);
    std::memcpy(mu, h->h_pack.p + (size_t)n * n, sizeof(double) * n);
    return EKF_OK;
  }
  if (int rc = check_internal(h, b, "ekf_download_state")) return rc;
  if (P) {
    // a destination in pinned host memory (what the Python binding hands out for large covariances: ekf_host_alloc) is
    // written by a kernel -- mirrored on the way, no SDMA copy (k_pack_dense); anything else by the mirror pass + rectangle copy
    // (up to 40 MB -- N = 1100: there the kernel is as fast as the copy engine at its best, 38 - 47 GB/s, and does not have
    //  the copy's bad days; beyond, the engine's larger PCIe payloads win: 54.6 against 49.8 GB/s at N = 2000.  tools/download_paths.py)
    const bool pack = h->opt_pack_dense == 2 || (h->opt_pack_dense == 1 && (size_t)n * n * sizeof(double) <= (40u << 20));
    double* dst = pack ? static_cast<double*>(device_view(P)) : nullptr;
    if (dst) {
      if (int rc = flush_pending(h)) return rc;    // the covariance is P_base + pending ranks, upper triangle
      launch_pack_dense(h->stream, h->dP.p + (size_t)b * h->pstride, h->ld, n, dst);
      HIP_TRY(h, hipGetLastError());
      h->dense_packs += 1;
    } else {
      if (int rc = materialize(h, b)) return rc;
      HIP_TRY(h, copy_cov(h, b, P, n, 0, 0, n, n, false));
    }
  }
  if (mu)
    HIP_TRY(h, hipMemcpyAsync(mu, h->dmu2[h->cur].p + (size_t)b * h->ld, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

extern "C" int ekf_download_block(ekf_handle* h, int b, int r0, int c0, int rows, int cols, double* out) {
  if (int rc = check_b(h, b, "ekf_download_block")) return rc;
  const int n = h->n[b];
  if (!out || rows <= 0 || cols <= 0 || r0 < 0 || c0 < 0 || r0 + rows > n || c0 + cols > n)
    return fail(h, EKF_ERR_ARG, "ekf_download_block: block outside the state");
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_internal(h, b, "ekf_download_block")) return rc;
  if (int rc = materialize(h, b)) return rc;
  HIP_TRY(h, copy_cov(h, b, out, cols, r0, c0, rows, cols, false));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

// The diagonal blocks of the covariance (k_marginals, ekf_marginals.hip); a read-only query, see query_begin.
extern "C" int ekf_download_marginals(ekf_handle* h, int b0, int count, double* pose, double* landmarks, int cap,
                                      int* n_landmarks) {
  const char* fn = "ekf_download_marginals";
  if (int rc = query_begin(h, fn, b0, count, nullptr, [&]() -> int {
        if (!pose) return bad_arg(h, fn, "NULL pose");
        int nl_hi = 0;
        for (int b = b0; b < b0 + count; ++b) nl_hi = std::max(nl_hi, (h->n[b] - 3) / 2);
        if (landmarks && cap < nl_hi)
          return bad_arg(h, fn, "cap " + std::to_string(cap) + " is below the largest landmark count " + std::to_string(nl_hi));
        return EKF_OK;
      }))
    return rc;
  if (!landmarks) cap = 0;
  Query q{};
  q.add(pose, (size_t)count * 9);
  q.add(landmarks, (size_t)count * (size_t)cap * 4);
  if (int rc = query_stage(h, q)) return rc;
  launch_marginals(h->stream, pending_view(h, b0, count), cap, q.out<double>(0), q.out<double>(1));
  if (int rc = query_end(h, fn, b0, count, q)) return rc;
  if (n_landmarks)
    for (int b = b0; b < b0 + count; ++b) n_landmarks[b - b0] = (h->n[b] - 3) / 2;
  return EKF_OK;
}

// Likelihood association of unlabelled observations (k_assoc_query / k_assoc_finish, ekf_associate.hip), under the measurement
// noise in effect; a read-only query, see query_begin.
extern "C" int ekf_associate(ekf_handle* h, int b0, int count, const double* range, const double* bearing, const int* m, int stride,
                             int* cand, double* cand_nis, double* cand_logdet, double* min_nis, double* all_nis, double* all_logdet,
                             int cap) {
  const char* fn = "ekf_associate";
  const bool full = all_nis != nullptr;
  AssocQueryPlan plan{};
  if (int rc = query_begin(h, fn, b0, count, nullptr, [&]() -> int {
        if (stride < 1 || stride > EKF_MMAX) return bad_arg(h, fn, "stride must lie in 1.." + std::to_string(EKF_MMAX));
        if (!range || !bearing || !m) return bad_arg(h, fn, "NULL observations");
        if (!cand) return bad_arg(h, fn, "NULL cand");
        if ((all_nis == nullptr) != (all_logdet == nullptr))
          return bad_arg(h, fn, "all_nis and all_logdet are given together or not at all");
        for (int bi = 0; bi < count; ++bi) {
          if (m[bi] < 0 || m[bi] > stride) return bad_arg(h, fn, "m[" + std::to_string(bi) + "] outside 0..stride");
          for (int q = 0; q < m[bi]; ++q)
            if (!std::isfinite(range[(size_t)bi * stride + q]) || !std::isfinite(bearing[(size_t)bi * stride + q]))
              return bad_arg(h, fn, "non-finite observation " + std::to_string(q) + " of trajectory " + std::to_string(b0 + bi));
        }
        plan = plan_assoc_query(h, b0, count, full ? std::max(cap, 0) : 0);
        if (full && cap < plan.nl_hi)
          return bad_arg(h, fn, "cap " + std::to_string(cap) + " is below the largest landmark count " + std::to_string(plan.nl_hi));
        return EKF_OK;
      }))
    return rc;
  if (!full) cap = 0;
  const size_t obs = (size_t)count * stride, full_words = obs * (size_t)cap;
  // inputs: range, bearing, m (ints, rounded up to doubles), the partial records
  const size_t m_words = ((size_t)count + 1) / 2;
  Query q{};
  q.plan.inputs = 2 * obs + m_words + (size_t)assoc_query_part_doubles(count, plan.chunks, stride);
  q.add(cand, obs);                                    // (2 ints per observation)
  q.add(cand_nis, obs * 2);
  q.add(cand_logdet, obs * 2);
  q.add(min_nis, obs);
  q.add(all_nis, full_words);
  q.add(all_logdet, full_words);
  if (int rc = query_stage(h, q)) return rc;
  double *dzr = h->dquery.p, *dzb = dzr + obs, *dpart = dzb + obs + m_words;
  int* dzm = reinterpret_cast<int*>(dzb + obs);
  HIP_TRY(h, hipMemcpyAsync(dzr, range, sizeof(double) * obs, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(dzb, bearing, sizeof(double) * obs, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(dzm, m, sizeof(int) * count, hipMemcpyHostToDevice, h->stream));
  launch_assoc_query(h->stream, pending_view(h, b0, count), h->dcfg, stride, cap, plan.chunks, dzr, dzb, dzm, dpart,
                     q.out<double>(4), q.out<double>(5), q.out<int>(0), q.out<double>(1), q.out<double>(2), q.out<double>(3));
  return query_end(h, fn, b0, count, q);
}

// The joint covariance and mean of the pose and a subset of landmarks (k_joint, ekf_joint.hip); a read-only query, see
// query_begin.
extern "C" int ekf_download_joint(ekf_handle* h, int b0, int count, const int* landmarks, const int* k, int stride, double* mean,
                                  double* cov) {
  const char* fn = "ekf_download_joint";
  JointQueryPlan jp{};
  if (int rc = query_begin(h, fn, b0, count, h && !cov ? "NULL cov" : nullptr, [&]() -> int {
        const char* why = plan_joint_query(h, b0, count, landmarks, k, stride, jp, h->joint_sel, h->joint_order);
        return why ? bad_arg(h, fn, why) : EKF_OK;
      }))
    return rc;
  const size_t mean_words = (size_t)count * jp.ns;
  Query q{};
  q.plan.inputs = (h->joint_sel.size() + 1) / 2;       // the selection (ints, rounded up to doubles)
  q.add(mean, mean_words);
  q.add(cov, mean_words * jp.ns);
  if (int rc = query_stage(h, q)) return rc;
  int* dsel = reinterpret_cast<int*>(h->dquery.p);
  HIP_TRY(h, hipMemcpyAsync(dsel, h->joint_sel.data(), sizeof(int) * h->joint_sel.size(), hipMemcpyHostToDevice, h->stream));
  launch_joint(h->stream, pending_view(h, b0, count), jp.ns, jp.nt, jp.tiles, dsel, q.out<double>(0), q.out<double>(1));
  return query_end(h, fn, b0, count, q);
}

// ---- the covariance's Cholesky factor (ekf_factor.hip) ----
static FactorView factor_view(const ekf_handle* h) { return FactorView{h->dfactor.p, h->factor.tstride, h->factor.lw, h->dfstat.p, h->dflog.p}; }
static int factor_drop(ekf_handle* h) {
  h->factor.held = false;
  RES_TRY(h, "the factor workspace", res::release_group<HipBackend>(h->stream, h->dfactor, h->dfstat, h->dflog));
  return EKF_OK;
}
// P = U^T U of trajectories [b0, b0 + count): the pending update applied, then the blocked factorisation into the handle's
// workspace; the filter itself is only read.
extern "C" int ekf_factor(ekf_handle* h, int b0, int count, double* logdet, int* info) {
  const char* fn = "ekf_factor";
  if (int rc = check_b(h, 0, fn)) return rc;
  if (int rc = check_range(h, fn, b0, count)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  // (as the downloads: the flags come back with one stream-ordered copy)
  HIP_TRY(h, hipMemcpyAsync(h->h_flags.p, h->dflags.p, sizeof(unsigned) * h->batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int b = b0; b < b0 + count; ++b)
    if (h->host_bad[b] || (h->h_flags.p[b] & EKF_FLAG_INTERNAL)) return check_internal(h, b, fn);
  if (int rc = flush_pending(h)) return rc;
  FactorPlan fp{};
  if (const char* why = plan_factor(h, b0, count, fp)) return bad_arg(h, fn, why);
  h->factor.held = false;                              // the workspace is about to be rewritten
  {
    const res::Status s0 = h->dfactor.reserve(fp.words, 0, h->stream);
    const res::Status s1 = s0.ok() ? h->dfstat.reserve(4 * (size_t)count, 4 * (size_t)h->batch, h->stream) : s0;
    const res::Status s2 = s1.ok() ? h->dflog.reserve((size_t)count, (size_t)h->batch, h->stream) : s1;
    if (!s2.ok()) {
      (void)hipGetLastError();
      (void)factor_drop(h);
      return res_fail(h, "ekf_factor: the factor workspace", s2);
    }
  }
  h->factor.b0 = b0;
  h->factor.count = count;
  h->factor.lw = fp.lw;
  h->factor.tstride = fp.tstride;
  h->factor.n.assign(h->n.begin() + b0, h->n.begin() + b0 + count);
  h->factor.info.assign((size_t)count, 0);
  h->factor_log.assign((size_t)count, 0.0);
  launch_factor(h->stream, pending_view(h, b0, count), factor_view(h), fp.nblk);
  HIP_TRY(h, hipGetLastError());
  std::vector<int>& st = h->factor_stat;
  st.assign(4 * (size_t)count, 0);
  HIP_TRY(h, hipMemcpyAsync(st.data(), h->dfstat.p, sizeof(int) * st.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->factor_log.data(), h->dflog.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int bi = 0; bi < count; ++bi) {
    h->factor.info[(size_t)bi] = st[4 * (size_t)bi];
    if (info) info[bi] = st[4 * (size_t)bi];
    if (logdet) logdet[bi] = st[4 * (size_t)bi] ? std::numeric_limits<double>::quiet_NaN() : h->factor_log[(size_t)bi];
  }
  h->factor.held = true;
  return EKF_OK;
}

// U^-T rhs (solve) or U^T z (multiply) for trajectories [b0, b0 + count) of the factored range.  The operand is uploaded into
// the queries' staging buffer, the result formed beside it and copied out.
static int factor_apply(ekf_handle* h, const char* fn, bool solve, int b0, int count, const double* x, int nrhs, int stride,
                        double* out, double* quad) {
  if (!h) return EKF_ERR_ARG;
  bool state = false;
  int nblk_hi = 0;
  if (const char* why = plan_factor_apply(h, h->factor, b0, count, x, nrhs, stride, &state, &nblk_hi))
    return state ? fail(h, EKF_ERR_STATE, std::string(fn) + ": " + why) : bad_arg(h, fn, why);
  if (!out && !(solve && quad)) return bad_arg(h, fn, "NULL output");
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t words = (size_t)count * (size_t)nrhs * (size_t)stride, qwords = (size_t)count * (size_t)nrhs;
  RES_TRY(h, "the queries' staging buffer", h->dquery.reserve(2 * words + qwords, 0, h->stream));
  double *dx = h->dquery.p, *dout = dx + words, *dquad = dout + words;
  HIP_TRY(h, hipMemcpyAsync(dx, x, sizeof(double) * words, hipMemcpyHostToDevice, h->stream));
  const int f0 = b0 - h->factor.b0;
  if (solve)
    launch_factor_solve(h->stream, factor_view(h), f0, count, nblk_hi, dx, nrhs, stride, dout, dquad);
  else
    launch_factor_multiply(h->stream, factor_view(h), f0, count, nblk_hi, dx, nrhs, stride, dout);
  HIP_TRY(h, hipGetLastError());
  if (out) HIP_TRY(h, hipMemcpyAsync(out, dout, sizeof(double) * words, hipMemcpyDeviceToHost, h->stream));
  if (solve && quad) HIP_TRY(h, hipMemcpyAsync(quad, dquad, sizeof(double) * qwords, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}
extern "C" int ekf_factor_solve(ekf_handle* h, int b0, int count, const double* rhs, int nrhs, int stride, double* white,
                                double* quad) {
  return factor_apply(h, "ekf_factor_solve", true, b0, count, rhs, nrhs, stride, white, quad);
}
extern "C" int ekf_factor_multiply(ekf_handle* h, int b0, int count, const double* z, int nrhs, int stride, double* out) {
  return factor_apply(h, "ekf_factor_multiply", false, b0, count, z, nrhs, stride, out, nullptr);
}

extern "C" int ekf_download_factor(ekf_handle* h, int b, double* U, int n) {
  const char* fn = "ekf_download_factor";
  if (!h) return EKF_ERR_ARG;
  if (!U) return bad_arg(h, fn, "NULL U");
  if (b < 0 || b >= h->batch) return bad_arg(h, fn, "trajectory index out of range");
  const FactorHeld& fh = h->factor;
  if (!fh.held) return fail(h, EKF_ERR_STATE, std::string(fn) + ": no factor is held (ekf_factor)");
  if (b < fh.b0 || b >= fh.b0 + fh.count) return fail(h, EKF_ERR_STATE, std::string(fn) + ": trajectory outside the factored range");
  const size_t bi = (size_t)(b - fh.b0);
  if (n != fh.n[bi]) return bad_arg(h, fn, "n does not match the factored n");
  if (fh.info[bi] != 0)
    return fail(h, EKF_ERR_STATE, std::string(fn) + ": the covariance of trajectory " + std::to_string(b) +
                                      " is not positive definite (info = " + std::to_string(fh.info[bi]) + ")");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpy2DAsync(U, sizeof(double) * (size_t)n, h->dfactor.p + bi * fh.tstride, sizeof(double) * (size_t)fh.lw,
                              sizeof(double) * (size_t)n, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

extern "C" int ekf_factor_release(ekf_handle* h) {
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  return factor_drop(h);
}

// ---- the log rings: the pose log (ekf_pose_log.hip) and the innovation log (ekf_innovations.hip) ----
// A ring is one or two device arrays of `capacity` step rows, `row_bytes` per (step, trajectory).  ring_resize replaces it by
// an empty one (capacity 0: switches the log off); `cap` and `steps` are the log's capacity and its count of logged steps.
// Each array is given as res::want(buffer, elements per (step, trajectory)).
template <class... Bufs>
static int ring_resize(ekf_handle* h, const char* fn, int capacity, int* cap, long long* steps, res::Want<Bufs>... arrays) {
  if (capacity < 0) return bad_arg(h, fn, "capacity must be >= 0");
  const size_t rows = (size_t)capacity * h->batch;
  if ((... || (rows * arrays.n * sizeof(*arrays.buf->p) > ((size_t)1 << 36)))) return bad_arg(h, fn, "the ring would exceed 64 GiB");
  HIP_TRY(h, hipSetDevice(h->device));
  // (launches in flight still write the old ring: release_group waits for the stream)
  RES_TRY(h, fn, res::release_group<HipBackend>(h->stream, *arrays.buf...));
  *cap = 0;
  *steps = 0;
  if (capacity == 0) return EKF_OK;
  const res::Status st = res::ensure_group(nullptr, res::want(*arrays.buf, rows * arrays.n)...);
  if (!st.ok()) {
    (void)hipGetLastError();
    return res_fail(h, (std::string(fn) + ": the ring of " + std::to_string(capacity) + " steps").c_str(), st);
  }
  *cap = capacity;
  return EKF_OK;
}
// Steps [first, first + count) must be among the last `cap` of the `steps` logged.
static int check_ring_range(ekf_handle* h, const char* fn, long long first, int count, long long steps, int cap) {
  if (ring_range_ok(first, count, steps, cap)) return EKF_OK;
  return bad_arg(h, fn, "steps [" + std::to_string(first) + ", " + std::to_string(first + count) + ") are not among the last " +
                            std::to_string(cap) + " of the " + std::to_string(steps) + " logged");
}

extern "C" int ekf_log_poses(ekf_handle* h, int capacity) {
  if (!h) return EKF_ERR_ARG;
  return ring_resize(h, "ekf_log_poses", capacity, &h->pose_cap, &h->pose_steps, res::want(h->dpose, POSE_ROW));
}

extern "C" int ekf_pose_steps(ekf_handle* h, long long* logged) {
  if (!h || !logged) return EKF_ERR_ARG;
  *logged = h->pose_steps;
  return EKF_OK;
}

// The block is returned exactly symmetric: its upper triangle, mirrored.
extern "C" int ekf_download_poses(ekf_handle* h, long long first, int count, double* pose, double* cov) {
  if (!h) return EKF_ERR_ARG;
  if (!h->dpose.p) return fail(h, EKF_ERR_STATE, "ekf_download_poses: the pose log is off (ekf_log_poses)");
  if (int rc = check_ring_range(h, "ekf_download_poses", first, count, h->pose_steps, h->pose_cap)) return rc;
  if (count > 0 && !pose) return fail(h, EKF_ERR_ARG, "ekf_download_poses: NULL pose");
  HIP_TRY(h, hipSetDevice(h->device));
  const long B = h->batch;
  std::vector<double> hr((size_t)count * B * POSE_ROW);
  const RingPieces rp = ring_pieces(first, count, h->pose_cap);
  for (int i = 0; i < rp.n; ++i) {
    const RingPieces::Piece& c = rp.piece[i];
    HIP_TRY(h, hipMemcpyAsync(hr.data() + c.done * B * POSE_ROW, h->dpose.p + c.slot * B * POSE_ROW, sizeof(double) * c.rows * B * POSE_ROW,
                              hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t q = 0; q < (size_t)count * B; ++q) {
    const double* r = hr.data() + q * POSE_ROW;
    for (int i = 0; i < 3; ++i) pose[q * 3 + i] = r[i];
    if (cov)
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) cov[q * 9 + 3 * i + j] = r[3 + 3 * std::min(i, j) + std::max(i, j)];
  }
  return EKF_OK;
}

extern "C" int ekf_log_innovations(ekf_handle* h, int capacity) {
  if (!h) return EKF_ERR_ARG;
  return ring_resize(h, "ekf_log_innovations", capacity, &h->innov_cap, &h->innov_steps, res::want(h->dinnov, AMAX),
                     res::want(h->dinnov_m, 1));
}

extern "C" int ekf_innovation_steps(ekf_handle* h, long long* logged) {
  if (!h || !logged) return EKF_ERR_ARG;
  *logged = h->innov_steps;
  return EKF_OK;
}

// Steps [first, first + count) of the log: copies of their ring rows (one or two pieces each: the ring may wrap), behind
// everything enqueued, into hm (count x batch counts) and hr (count x batch x AMAX entries).  Runs nothing else on the device.
static int read_log(ekf_handle* h, long long first, int count, const char* fn, std::vector<int>& hm, std::vector<InnovRec>& hr) {
  if (!h->dinnov.p) return fail(h, EKF_ERR_STATE, std::string(fn) + ": the innovation log is off (ekf_log_innovations)");
  if (int rc = check_ring_range(h, fn, first, count, h->innov_steps, h->innov_cap)) return rc;
  const int B = h->batch;
  hm.resize((size_t)count * B);
  hr.resize((size_t)count * B * AMAX);
  HIP_TRY(h, hipSetDevice(h->device));
  const RingPieces rp = ring_pieces(first, count, h->innov_cap);
  for (int i = 0; i < rp.n; ++i) {
    const RingPieces::Piece& c = rp.piece[i];
    HIP_TRY(h, hipMemcpyAsync(hm.data() + c.done * B, h->dinnov_m.p + c.slot * B, sizeof(int) * c.rows * B, hipMemcpyDeviceToHost,
                              h->stream));
    HIP_TRY(h, hipMemcpyAsync(hr.data() + c.done * B * AMAX, h->dinnov.p + c.slot * B * AMAX, sizeof(InnovRec) * c.rows * B * AMAX,
                              hipMemcpyDeviceToHost, h->stream));
  }
  return check_internal(h, -1, fn);                    // (synchronises: the copies above are done)
}

// The entries beyond a step's count are set here.
extern "C" int ekf_download_innovations(ekf_handle* h, long long first, int count, int* m, int* idx, double* y, double* S,
                                        double* nis) {
  if (!h) return EKF_ERR_ARG;
  if (count > 0 && !m && h->dinnov.p) return fail(h, EKF_ERR_ARG, "ekf_download_innovations: NULL m");
  std::vector<int> hm;
  std::vector<InnovRec> hr;
  if (int rc = read_log(h, first, count, "ekf_download_innovations", hm, hr)) return rc;
  const int B = h->batch;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t e = 0; e < (size_t)count * B; ++e) {
    m[e] = hm[e];
    const int kept = std::min(hm[e], AMAX);
    for (int j = 0; j < AMAX; ++j) {
      const size_t q = e * AMAX + j;
      const InnovRec& r = hr[q];
      const bool on = j < kept;
      if (idx) idx[q] = on ? r.idx : -1;
      if (y)
        for (int k = 0; k < 2; ++k) y[2 * q + k] = on ? r.y[k] : nan;
      if (S)
        for (int k = 0; k < 4; ++k) S[4 * q + k] = on ? r.S[k] : nan;
      if (nis) nis[q] = on ? r.nis : nan;
    }
  }
  return EKF_OK;
}

extern "C" int ekf_download_innovation_rejections(ekf_handle* h, long long first, int count, int* rejected) {
  if (!h) return EKF_ERR_ARG;
  if (count > 0 && !rejected && h->dinnov.p) return fail(h, EKF_ERR_ARG, "ekf_download_innovation_rejections: NULL rejected");
  std::vector<int> hm;
  std::vector<InnovRec> hr;
  if (int rc = read_log(h, first, count, "ekf_download_innovation_rejections", hm, hr)) return rc;
  for (size_t e = 0; e < (size_t)count * h->batch; ++e) {
    const int kept = std::min(hm[e], AMAX);
    for (int j = 0; j < AMAX; ++j) rejected[e * AMAX + j] = j < kept ? hr[e * AMAX + j].rejected : -1;
  }
  return EKF_OK;
}

// ---- the NIS gate (solve kernels: ekf_kernels.hip solve_body, ekf_cadence.hip k_solve_cad, ekf_small.hip small_step) ----
extern "C" int ekf_set_nis_gate(ekf_handle* h, double threshold) {
  if (!h) return EKF_ERR_ARG;
  if (!(threshold > 0.0))                              // (NaN too)
    return fail(h, EKF_ERR_ARG, "ekf_set_nis_gate: the threshold must be > 0 (INFINITY: off)");
  HIP_TRY(h, hipSetDevice(h->device));
  const bool on = !std::isinf(threshold);
  if (on) RES_TRY(h, "the NIS gate's counters", h->dgate.ensure((size_t)h->batch));
  // (stream-ordered behind every launch enqueued so far, which may still count rejections under the old threshold)
  if (h->dgate.p) HIP_TRY(h, hipMemsetAsync(h->dgate.p, 0, sizeof(unsigned long long) * h->batch, h->stream));
  h->dcfg.nis_gate = threshold;
  h->dcfg.gate_rej = on ? h->dgate.p : nullptr;
  return EKF_OK;
}

// ---- per-trajectory noise constants (solve kernels: ekf_kernels.hip solve_body, ekf_cadence.hip k_solve_cad, ekf_small.hip
// small_step) ----
// Row of the table for motion sigma s and measurement sigma q: the expressions ekf_create folds the handle's config with, so
// that a row of the handle's own sigmas is the same doubles as dcfg.rd / dcfg.qd.
static void noise_row_of(double s, double q, double* r) {
  r[0] = s * s;                                        // src/replay_no_ros.py:421
  r[1] = s * s;
  r[2] = (s / 2) * (s / 2);
  r[3] = q * q;                                        // :438
  r[4] = q * q;
}

extern "C" int ekf_set_noise(ekf_handle* h, int b0, int count, const double* motion_sigma, const double* meas_sigma) {
  if (int rc = check_range(h, "ekf_set_noise", b0, count)) return rc;
  for (int i = 0; i < count; ++i) {
    if (motion_sigma && !std::isfinite(motion_sigma[i]))
      return fail(h, EKF_ERR_ARG, "ekf_set_noise: motion_sigma[" + std::to_string(i) + "] is not finite");
    if (motion_sigma && motion_sigma[i] < 0.0)
      return fail(h, EKF_ERR_ARG, "ekf_set_noise: motion_sigma[" + std::to_string(i) + "] < 0");
    if (meas_sigma && !std::isfinite(meas_sigma[i]))
      return fail(h, EKF_ERR_ARG, "ekf_set_noise: meas_sigma[" + std::to_string(i) + "] is not finite");
    if (meas_sigma && !(meas_sigma[i] > 0.0))          // (Q > 0 keeps S invertible: ekf_devfn.h)
      return fail(h, EKF_ERR_ARG, "ekf_set_noise: meas_sigma[" + std::to_string(i) + "] <= 0");
  }
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t B = (size_t)h->batch;
  if (h->noise_ms.empty()) {
    h->noise_ms.assign(B, h->cfg.motion_sigma);
    h->noise_qs.assign(B, h->cfg.meas_sigma);
  }
  for (int i = 0; i < count; ++i) {
    h->noise_ms[(size_t)b0 + i] = motion_sigma ? motion_sigma[i] : h->cfg.motion_sigma;
    h->noise_qs[(size_t)b0 + i] = meas_sigma ? meas_sigma[i] : h->cfg.meas_sigma;
  }
  // the table is on while some row differs from the handle's constants; off, every kernel is the one without it
  std::vector<double> rows(B * NOISE_ROW);
  bool differs = false;
  for (size_t b = 0; b < B; ++b) {
    double* r = rows.data() + b * NOISE_ROW;
    noise_row_of(h->noise_ms[b], h->noise_qs[b], r);
    differs |= r[0] != h->dcfg.rd[0] || r[1] != h->dcfg.rd[1] || r[2] != h->dcfg.rd[2] || r[3] != h->dcfg.qd[0] ||
               r[4] != h->dcfg.qd[1];
  }
  if (!differs) {
    h->dcfg.noise = nullptr;
    return EKF_OK;
  }
  // (stream-ordered: launches enqueued before read the old rows, those enqueued after the new ones; every launch that reads
  // the table is on h->stream.  begin waits until the previous upload out of the pinned copy has run)
  double* stage = nullptr;
  RES_TRY(h, "the noise table", h->noise.begin(rows.size(), 0, h->stream, &stage));
  std::memcpy(stage, rows.data(), sizeof(double) * rows.size());
  RES_TRY(h, "the noise table's upload", h->noise.commit(rows.size(), h->stream));
  h->dcfg.noise = h->noise.device();
  return EKF_OK;
}

extern "C" int ekf_get_noise(ekf_handle* h, int b0, int count, double* motion_sigma, double* meas_sigma) {
  if (int rc = check_range(h, "ekf_get_noise", b0, count)) return rc;
  for (int i = 0; i < count; ++i) {
    const size_t b = (size_t)b0 + i;
    if (motion_sigma) motion_sigma[i] = h->noise_ms.empty() ? h->cfg.motion_sigma : h->noise_ms[b];
    if (meas_sigma) meas_sigma[i] = h->noise_qs.empty() ? h->cfg.meas_sigma : h->noise_qs[b];
  }
  return EKF_OK;
}

extern "C" int ekf_download_gate_counts(ekf_handle* h, int b0, int count, long long* rejected) {
  if (int rc = check_range(h, "ekf_download_gate_counts", b0, count)) return rc;
  if (!rejected) return fail(h, EKF_ERR_ARG, "ekf_download_gate_counts: NULL rejected");
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<unsigned long long> hc((size_t)count, 0ull);
  if (h->dgate.p)
    HIP_TRY(h, hipMemcpyAsync(hc.data(), h->dgate.p + b0, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost, h->stream));
  if (int rc = check_internal(h, -1, "ekf_download_gate_counts")) return rc;   // (synchronises: the copy above is done)
  for (int b = 0; b < count; ++b) rejected[b] = (long long)hc[b];
  return EKF_OK;
}

extern "C" int ekf_download_mean(ekf_handle* h, int b, double* mu, int n) {
  return ekf_download_state(h, b, mu, nullptr, n);
}

extern "C" int ekf_state_size(ekf_handle* h, int b, int* n) {
  if (int rc = check_b(h, b, "ekf_state_size")) return rc;
  if (!n) return fail(h, EKF_ERR_ARG, "ekf_state_size: NULL");
  *n = h->n[b];
  return EKF_OK;
}

extern "C" int ekf_add_landmarks(ekf_handle* h, int b, int first_index, const double* xy, int k) {
  if (int rc = check_b(h, b, "ekf_add_landmarks")) return rc;
  if (k <= 0) return EKF_OK;
  if (!xy) return fail(h, EKF_ERR_ARG, "ekf_add_landmarks: NULL xy");
  const int n_old = h->n[b], n_new = n_old + 2 * k;
  if (first_index != (n_old - 3) / 2)
    return fail(h, EKF_ERR_ARG, "ekf_add_landmarks: first_index must continue the landmark count (replay_no_ros.py:294-295)");
  if (n_new > h->n_max) return fail(h, EKF_ERR_ARG, "ekf_add_landmarks: state would exceed n_max");
  if (2 * k > 2 * h->ld) return fail(h, EKF_ERR_ARG, "ekf_add_landmarks: too many landmarks in one call");
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = flush_pending(h)) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // xy is staged through a single scratch buffer
  HIP_TRY(h, hipMemcpyAsync(h->dscratch.p, xy, sizeof(double) * 2 * k, hipMemcpyHostToDevice, h->stream));
  launch_add_landmarks(h->stream, h->dP.p + (size_t)b * h->pstride, h->dmu2[h->cur].p + (size_t)b * h->ld, h->ld, n_old, n_new,
                       h->cfg.landmark_init_var, h->dscratch.p);
  HIP_TRY(h, hipGetLastError());
  if (int rc = set_size(h, b, n_new)) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

// Marginalise landmarks out (k_remove, ekf_remove.hip): apply what is pending, compact P_base's stored triangle and the mean in
// place, then the bookkeeping -- sizes, active bound and its floor, the device tag table and the last window's tags, the
// uploaded stream (refused from now on).  b < 0: every trajectory, one launch.
extern "C" int ekf_remove_landmarks(ekf_handle* h, int b, const int* landmarks, int k) {
  if (!h) return EKF_ERR_ARG;
  if (int rc = (b < 0 ? refresh_sizes(h) : check_b(h, b, "ekf_remove_landmarks"))) return rc;
  const int b0 = b < 0 ? 0 : b, nb = b < 0 ? h->batch : 1;
  RemovePlan rp;
  if (const char* why = plan_remove(h, b0, nb, landmarks, k, rp)) return fail(h, EKF_ERR_ARG, why);
  if (k == 0) return EKF_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_internal(h, b, "ekf_remove_landmarks")) return rc;
  bool rm_fresh;
  RES_TRY(h, "ekf_remove_landmarks's tables",
          res::ensure_group(&rm_fresh, res::want(h->drm_tab, 2 * (size_t)h->ld), res::want(h->drm_flag, (size_t)h->ld * h->batch)));
  if (rm_fresh) HIP_TRY(h, hipMemsetAsync(h->drm_flag.p, 0, sizeof(unsigned) * (size_t)h->ld * h->batch, h->stream));
  if (int rc = flush_pending(h)) return rc;
  const size_t nt = rp.src.size();
  HIP_TRY(h, hipMemcpyAsync(h->drm_tab.p, rp.src.data(), sizeof(int) * nt, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->drm_tab.p + h->ld, rp.dst.data(), sizeof(int) * nt, hipMemcpyHostToDevice, h->stream));
  h->rm_seq += 1;
  if (h->rm_seq == 0) h->rm_seq = 1;                   // (0 is what the announcements start at)
  launch_remove(h->stream, bank_view(h), h->dmu2[h->cur].p, rp, h->drm_tab.p, h->drm_tab.p + h->ld, h->drm_flag.p, b0, nb, h->rm_seq);
  HIP_TRY(h, hipGetLastError());
  // the active bound loses the removed indices below it; everything at or beyond it was, and still is, uncorrelated
  for (int t = b0; t < b0 + nb; ++t) {
    int below = 0;
    for (int i = 0; i < k; ++i) below += (3 + 2 * landmarks[i] < h->neff[t]) ? 2 : 0;
    h->neff[t] -= below;
    h->neff_enq[t] = h->neff[t];
    h->n[t] -= rp.k2;
  }
  HIP_TRY(h, hipMemcpyAsync(h->dn.p, h->n.data(), sizeof(int) * h->batch, hipMemcpyHostToDevice, h->stream));
  if (int rc = push_floor(h, true)) return rc;
  // the device tag table (removed tags: -1, seen again = new) and the last window's tags_positions record, renumbered
  std::vector<int> tm;
  if (h->dtagmap.p) {
    tm.resize((size_t)TAGMAX * nb);
    HIP_TRY(h, hipMemcpyAsync(tm.data(), h->dtagmap.p + (size_t)b0 * TAGMAX, sizeof(int) * tm.size(), hipMemcpyDeviceToHost, h->stream));
  }
  std::vector<AssocOut> ao;
  if (h->d_assoc_out.p) {
    ao.resize(nb);
    HIP_TRY(h, hipMemcpyAsync(ao.data(), h->d_assoc_out.p + b0, sizeof(AssocOut) * nb, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  auto renum = [&](int lm) { return lm < 0 || 3 + 2 * lm >= (int)rp.dst.size() ? lm : (rp.dst[3 + 2 * lm] < 0 ? -1 : (rp.dst[3 + 2 * lm] - 3) / 2); };
  if (h->dtagmap.p) {
    for (int& v : tm) v = renum(v);
    HIP_TRY(h, hipMemcpyAsync(h->dtagmap.p + (size_t)b0 * TAGMAX, tm.data(), sizeof(int) * tm.size(), hipMemcpyHostToDevice, h->stream));
  }
  if (h->d_assoc_out.p) {
    for (AssocOut& a : ao) {
      int m = 0;
      for (int i = 0; i < std::min(a.m, AMAX); ++i) {
        const int lm = renum(a.idx[i]);
        if (lm < 0) continue;
        a.idx[m] = lm;
        a.tag_id[m] = a.tag_id[i];
        a.xw[m] = a.xw[i];
        a.yw[m] = a.yw[i];
        a.err[m] = a.err[i];
        a.range[m] = a.range[i];
        a.bearing[m] = a.bearing[i];
        ++m;
      }
      a.m = m;
      a.n_after = std::max(3, a.n_after - rp.k2);
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_assoc_out.p + b0, ao.data(), sizeof(AssocOut) * nb, hipMemcpyHostToDevice, h->stream));
  }
  if (h->stream_steps > 0) h->stream_stale = true;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return check_internal(h, b, "ekf_remove_landmarks");   // (a wait of k_remove that ran into its bound)
}

// ---- step machinery -------------------------------------------------------------------------
static int prof_event(ekf_handle* h, hipEvent_t* ev, int cls = 0) {
  if ((h->prof_used & 1) == 0) {
    if (h->prof_cls.size() <= h->prof_used / 2) h->prof_cls.resize(h->prof_used / 2 + 1);
    h->prof_cls[h->prof_used / 2] = cls;
  }
  if (h->prof_used == h->prof_pool.size()) h->prof_pool.emplace_back();
  Event& e = h->prof_pool[h->prof_used];
  RES_TRY(h, "a profiling event", e.ensure(true));
  h->prof_used += 1;
  *ev = e.ev;                                          // (the native handle: the pool may move its events when it grows)
  return EKF_OK;
}
// (diagnostic) an event pair around the launches between prof_open and prof_close on stream `st`, class `cls`
struct ProfBracket { hipEvent_t e1 = nullptr; hipStream_t st = nullptr; };
static int prof_open(ekf_handle* h, int cls, hipStream_t st, ProfBracket* pb) {
  pb->e1 = nullptr;
  if (!h->profile || !h->opt_profile_kernels) return EKF_OK;
  hipEvent_t e0;
  if (int rc = prof_event(h, &e0, cls)) return rc;
  if (int rc = prof_event(h, &pb->e1, cls)) return rc;
  pb->st = st;
  HIP_TRY(h, hipEventRecord(e0, st));
  return EKF_OK;
}
static int prof_close(ekf_handle* h, ProfBracket* pb) {
  if (pb->e1) HIP_TRY(h, hipEventRecord(pb->e1, pb->st));
  return EKF_OK;
}
// `launch()` inside such a pair
template <class Launch>
static int launch_profiled(ekf_handle* h, int cls, hipStream_t st, Launch launch) {
  ProfBracket pb;
  if (int rc = prof_open(h, cls, st, &pb)) return rc;
  launch();
  return prof_close(h, &pb);
}

// Apply the pending low-rank update to P_base:  P_base += W V + diag(dacc)  (one pass over P), on stream `st` (the
// handle's own unless the look-ahead of ekf_stream_run sends it to the second one).
static int flush_pending(ekf_handle* h, hipStream_t st, const CadOut* wv) {
  if (h->pending_k == 0) return EKF_OK;
  if (!st) st = h->stream;
  const PassPlan p = plan_pass(h);
  const int* shares = nullptr;
  if (p.kernel == 2 && p.long_few) {
    // build_pass_shares depends on the size only through the number of slabs and the last strip: with the active bound
    // on and a growing map the bound changes at almost every pass, the table only when it crosses a strip
    const int nrb = (p.e_hi + 127) / 128, s_last = (p.e_hi - 1) >> 6;
    const int key[4] = {h->batch, nrb, s_last, p.rs_workgroups};
    if (std::memcmp(key, h->shares_key, sizeof key) != 0) {
      const size_t words = (size_t)h->cu_count * pass_share_pieces() * 4;
      const int nb = h->shares_cur ^ 1;
      // (the pinned copy is free once its previous upload has been executed: two tables back, long ago)
      int* table = nullptr;
      bool fresh;
      RES_TRY(h, "the pass's share table", h->shares2[nb].begin(words, 0, st, &table, &fresh));
      if (fresh) std::memset(table, 0, sizeof(int) * words);
      h->shares_ok = build_pass_shares(h->batch, p.e_hi, p.rs_workgroups, table);
      if (h->shares_ok > 0) order_pass_shares(p.rs_workgroups, pass_share_pieces(), table, words);
      // stream-ordered: the launch below, on the same stream, reads the table after the copy; the pass that read the
      // other table -- possibly still running on the handle's other stream -- is not touched
      RES_TRY(h, "the share table's upload", h->shares2[nb].commit(words, st));
      h->shares_cur = nb;
      std::memcpy(h->shares_key, key, sizeof key);
    }
    if (h->shares_ok > 0) shares = h->shares2[h->shares_cur].device();
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  // (profiling: every `profile_stride`-th launch of the pass is bracketed by an event pair -- a record costs its stream ~6 us)
  const bool timed = h->profile && (h->prof_seen++ % h->profile_stride) == 0;
  if (timed) {
    if (int rc = prof_event(h, &e0)) return rc;
    if (int rc = prof_event(h, &e1)) return rc;
    HIP_TRY(h, hipEventRecord(e0, st));
  }
  h->last_kernel = p.kernel;
  h->last_wv = (p.kernel == 2 && wv) ? 1 : 0;
  h->last_nkt = p.nkt;
  h->last_streaming = p.streaming ? 1 : 0;
  h->last_shares = shares ? h->shares_ok : 0;
  if (p.kernel == 2)                                   // (the step before left the queue heads at zero)
    launch_flush_rs(st, p, bank_view(h), step_bufs(h).dacc_in, shares, wv);
  else
    launch_flush(st, p, bank_view(h), step_bufs(h).dacc_in);
  if (timed) HIP_TRY(h, hipEventRecord(e1, st));
  HIP_TRY(h, hipGetLastError());
  h->pending_k = 0;                                    // (with no rank pending k_solve takes the pending noise as zero: no clearing)
  h->pending_steps = 0;
  return EKF_OK;
}
static int flush_pending(ekf_handle* h) { return flush_pending(h, nullptr); }

// ---- the rank fronts: ekf_update_direct (k_direct) and ekf_update_linear (k_linear; ekf_rank_front.h) ----
// Each call is check_b (which refreshes the sizes a device-side association grew), its plan function, front_run with its pack
// function and launcher, front_read.  front_run: the trajectories of the range must be defined; room for the launch's table
// `tab` (ekf_host_plan.h: FrontTable); what is pending is applied, so that the front reads P_base; `pack` fills h->front_ints /
// front_dbls for the bank (behind the flush: pack_linear raises the bounds).  Where a trajectory brings rows (kpad > 0): the
// two uploads, `launch(plan, meas, out)` in a profile bracket of class `cls`, the results' copy, and the covariance pass on the
// ranks the front left, as on any pending ranks, over the bounds it left -- the launch covers the bank: it leaves each
// trajectory's active bound where the pass reads it (dso[b].neff may be stale, e.g. behind an upload; neff_enq mirrors it
// for the planner from the table's bound column) and zeroes the pending pose noise the pass adds.  Ends in the call's one
// synchronise: the results are in h->front_out.
template <class Pack, class Launch>
static int front_run(ekf_handle* h, const char* fn, int b0, int count, const FrontTable& tab, int cls, int kpad, Pack pack,
                     Launch launch) {
  HIP_TRY(h, hipSetDevice(h->device));
  for (int b = b0; b < b0 + count; ++b)
    if (int rc = check_internal(h, b, fn)) return rc;
  const size_t B = (size_t)h->batch;
  RES_TRY(h, (std::string(fn) + "'s tables").c_str(), h->dfront.reserve(tab.words(B), 0, h->stream));
  if (int rc = flush_pending(h)) return rc;
  pack();
  h->front_out.assign(2 * B, 0.0);
  if (kpad > 0) {
    int* dplan = reinterpret_cast<int*>(h->dfront.p);
    double* dmeas = h->dfront.p + tab.int_words(B);
    double* dout = dmeas + B * tab.dbls;
    HIP_TRY(h, hipMemcpyAsync(dplan, h->front_ints.data(), sizeof(int) * h->front_ints.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dmeas, h->front_dbls.data(), sizeof(double) * h->front_dbls.size(), hipMemcpyHostToDevice, h->stream));
    if (int rc = launch_profiled(h, cls, h->stream, [&] { launch(dplan, dmeas, dout); })) return rc;
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->front_out.data(), dout, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, h->stream));
    for (size_t b = 0; b < B; ++b) h->neff_enq[b] = h->front_ints[b * tab.ints + 1];
    h->pending_k = kpad;
    if (int rc = flush_pending(h)) {
      for (int b = b0; b < b0 + count; ++b) h->host_bad[b] = 1;       // (the mean has moved, the covariance has not)
      return rc;
    }
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}
// what the front found for the trajectories of the range, D[bi] rows each: a trajectory without rows has NIS 0 and is not applied
static void front_read(const ekf_handle* h, int b0, int count, const std::vector<int>& D, double* nis, int* dof, int* applied) {
  for (int bi = 0; bi < count; ++bi) {
    const bool any = D[bi] > 0;
    if (nis) nis[bi] = any ? h->front_out[2 * (size_t)(b0 + bi)] : 0.0;
    if (dof) dof[bi] = D[bi];
    if (applied) applied[bi] = any && h->front_out[2 * (size_t)(b0 + bi) + 1] != 0.0 ? 1 : 0;
  }
}

// Direct measurements: V = P[s, :], W = -(S^-1 V)^T, zeros for every trajectory that brings nothing or is rejected.
extern "C" int ekf_update_direct(ekf_handle* h, int b0, int count, const int* target, const double* z, const double* R,
                                 const int* m, int stride, const double* gate, double* nis, int* dof, int* applied) {
  const char* fn = "ekf_update_direct";
  if (int rc = check_b(h, 0, fn)) return rc;
  DirectPlan& dp = h->direct_plan;
  if (const char* why = plan_direct(h, b0, count, target, z, R, m, stride, gate, dp)) return bad_arg(h, fn, why);
  if (int rc = front_run(
          h, fn, b0, count, direct_table(), 4, dp.kpad,
          [&] { pack_direct(h, dp, b0, count, z, R, m, stride, gate, h->front_ints, h->front_dbls); },
          [&](const int* dplan, const double* dmeas, double* dout) {
            launch_direct(h->stream, front_rows_cap(dp.kpad, DIRECT_ROWS), bank_view(h), h->ddacc2[h->dcur].p, h->dmu2[h->cur].p, dplan,
                          dmeas, dout, dp.kpad);
          }))
    return rc;
  front_read(h, b0, count, dp.D, nis, dof, applied);
  return EKF_OK;
}

// Linear measurements: a dense H over a small sub-state, V = H_s P[s, :], W = -(S^-1 V)^T.  Unlike a direct fix a general row
// correlates its targets: pack_linear first raises the active bound of every trajectory that brings rows over its sub-state.
extern "C" int ekf_update_linear(ekf_handle* h, int b0, int count, const int* landmarks, const int* k, int lstride, const double* H,
                                 const double* r, const double* R, const int* d, int dstride, int innovation, const double* gate,
                                 double* nis, int* applied) {
  const char* fn = "ekf_update_linear";
  if (int rc = check_b(h, 0, fn)) return rc;
  LinearPlan& lp = h->linear_plan;
  if (const char* why = plan_linear(h, b0, count, landmarks, k, lstride, H, r, R, d, dstride, gate, lp)) return bad_arg(h, fn, why);
  const int cap = front_rows_cap(lp.kpad, LINEAR_ROWS), nsl = 3 + 2 * lstride;
  if (int rc = front_run(
          h, fn, b0, count, linear_table(cap, nsl), 5, lp.kpad,
          [&] { pack_linear(h, lp, b0, count, lstride, H, r, R, dstride, gate, h->front_ints, h->front_dbls); },
          [&](const int* dplan, const double* dmeas, double* dout) {
            launch_linear(h->stream, cap, bank_view(h), h->ddacc2[h->dcur].p, h->dmu2[h->cur].p, dplan, dmeas, dout, lp.kpad, nsl,
                          innovation ? 1 : 0);
          }))
    return rc;
  front_read(h, b0, count, lp.D, nis, nullptr, applied);
  return EKF_OK;
}

// The small-state path (ekf_small.hip, ekf_host_plan.h: small_path): `nsteps` steps per trajectory in one launch.
static int enqueue_small(ekf_handle* h, const StepIn* d_in, int nsteps) {
  const int n_hi = bank_n_hi(h, true);
  const int out_b = h->fetch_b;                        // (ekf_step_fetch, last pass of its step: see there)
  h->fetch_b = -1;
  // (this path writes the log itself, and applies the NIS gate and the noise table in the same instantiations)
  const bool logged = h->dinnov.p && h->lg_slot >= 0;
  const InnovLog lg = logged ? innov_log(h, h->lg_slot, h->lg_jbase) : InnovLog{};
  // (the pose log likewise: every pass of a step writes the step's row, the last one last)
  const bool posed = h->dpose.p && h->pl_slot >= 0;
  const PoseLog plg = posed ? pose_log(h, h->pl_slot) : PoseLog{};
  SmallFetch fetch;
  if (out_b >= 0) fetch = SmallFetch{h->h_pack.p, out_b, reinterpret_cast<unsigned long long*>(h->h_pack.p + PACK_WORDS - 1), ++h->fetch_seq};
  if (launch_small_stream(h->stream, bank_view(h), step_bufs(h), d_in, nsteps, h->dcfg, n_hi, plan_small(h, n_hi), fetch,
                          logged || h->dcfg.gate_rej || h->dcfg.noise ? &lg : nullptr, posed ? &plg : nullptr) != 0)
    return fail(h, EKF_ERR_HIP, "small-state launch: hipFuncSetAttribute failed");
  HIP_TRY(h, hipGetLastError());
  h->fetched = out_b >= 0;
  h->cur ^= 1;
  h->small_launches += 1;
  return EKF_OK;
}

// The innovation log of a per-step pass: its records (h->dso.p) copied out right behind its solve, before the next solve reuses them.
static void log_pass(ekf_handle* h, const StepIn* d_in) {
  if (!h->dinnov.p || h->lg_slot < 0) return;
  launch_innov_step(h->stream, d_in, h->dso.p, h->dcfg.enable_measurement_model, h->dcfg.gate_rej != nullptr, h->batch,
                    innov_log(h, h->lg_slot, h->lg_jbase));
}

// The pose log's row of a step that ran on the per-step kernels: formed from what is in memory behind the step's last pass
// (k_pose_step: the new mean, P_base, the pending ranks and noise, as ekf_download_marginals reads them).  The small-state
// path has written the row itself.
static int log_pose_step(ekf_handle* h) {
  if (!h->dpose.p || h->pl_slot < 0 || small_path(h)) return EKF_OK;
  launch_pose_step(h->stream, pending_view(h, 0, h->batch), pose_log(h, h->pl_slot));
  HIP_TRY(h, hipGetLastError());
  return EKF_OK;
}

// Enqueue one device pass with inputs already at d_in (StepIn[batch]); m_hi = max m over the batch.
static int enqueue_pass(ekf_handle* h, const StepIn* d_in, int m_hi) {
  if (small_path(h)) return enqueue_small(h, d_in, 1);
  const int n_hi = bank_n_hi(h, true);
  const StepPlan sp = plan_step(h, m_hi, n_hi);
  const BankView bank = bank_view(h);
  const StepBufs bufs = step_bufs(h);
  if (sp.form == STEP_PREDICT) {
    // prediction only, nothing pending: rows/cols 0,1 of P_base directly, O(n)
    launch_solve(h->stream, bank, bufs, StepArgs{d_in, h->dfac.p, h->dfloor.p, 0}, h->dcfg);
    launch_predict_rc(h->stream, bank, bufs, n_hi);
    log_pass(h, d_in);
    // k_predict_rc applied the noise itself (and nothing reads the pending-noise buffers while no rank is pending)
    HIP_TRY(h, hipGetLastError());
    h->cur ^= 1;
    return EKF_OK;
  }
  if (sp.flush_before)
    if (int rc = flush_pending(h)) return rc;
  StepArgs sa{d_in, h->dfac.p, h->dfloor.p, h->pending_k};
  if (sp.form == STEP_SPLIT || sp.form == STEP_SPLIT_TP) {
    sa.mbox = h->dmbox.p;                                // (the throughput shape's; k_step_split has none)
    sa.ready = h->dready.p, sa.seq = ++h->step_seq, sa.publish = h->opt_fused_step == 1;
    if (sp.form == STEP_SPLIT) launch_step_split(h->stream, sp.mcap, bank, bufs, sa, h->dcfg, n_hi);
    else launch_step_split_tp(h->stream, sp.mcap, bank, bufs, sa, h->dcfg, n_hi);
  } else {
    launch_solve(h->stream, bank, bufs, sa, h->dcfg);
    launch_panels(h->stream, sp.mcap, sp.panels_latency, bank, bufs, h->dfac.p, n_hi);
  }
  log_pass(h, d_in);
  HIP_TRY(h, hipGetLastError());
  h->dcur ^= 1;
  h->cur ^= 1;
  h->pending_k += 2 * m_hi;
  h->pending_steps += 1;
  if (pass_due_after_step(h, m_hi))
    if (int rc = flush_pending(h)) return rc;
  return EKF_OK;
}

// The plan of a run's cadences (h->run_plan) to the device: stream-ordered out of pinned memory, no host synchronisation.
static int upload_run_plan(ekf_handle* h) {
  const size_t count = h->run_plan.entries.size();
  const int nb = h->plan_cur ^ 1;
  // (the pinned copy is free once its previous upload has been executed: two runs back.  A copy that is too small is replaced
  //  once the stream is idle: kernels of an earlier run may still read the old device copy)
  CadPlan* stage = nullptr;
  RES_TRY(h, "the run plan", h->plan2[nb].begin(count, (size_t)64 * h->batch, h->stream, &stage));
  std::memcpy(stage, h->run_plan.entries.data(), sizeof(CadPlan) * count);
  RES_TRY(h, "the run plan's upload", h->plan2[nb].commit(count, h->stream));
  h->plan_cur = nb;
  return EKF_OK;
}

// What a planned piece of a run needs before its first cadence (h->run_plan holds the piece): whether its solves are chained --
// decided per piece; whether a cadence is chained to the next is decided where the pass between them is planned
// (plan_cadence_step) -- and everything a cadence touches: the chained set is one group; it shares the records and the block
// buffer with the look-ahead's set, whose block buffer is allocated where a look-ahead first runs (enqueue_cadence).
static int prepare_piece(ekf_handle* h) {
  h->chain_run = plan_chain_run(h, h->run_plan.ncad);
  h->chain_gw = chain_gather_workgroups(h->batch, h->cu_count);
  const size_t B = (size_t)h->batch;
  if (!h->chain_run) {
    RES_TRY(h, "the cadence records", res::ensure_group(nullptr, res::want(h->dcad2[0], B), res::want(h->dcad2[1], B)));
    return EKF_OK;
  }
  const size_t gw = B * 84 * 88;
  bool fresh;
  RES_TRY(h, "the chained run's buffers",
          res::ensure_group(&fresh, res::want(h->dcad2[0], B), res::want(h->dcad2[1], B),
                            res::want(h->dgbuf, (size_t)cadence_gbuf_doubles() * B),
                            res::want(h->dprow3[0], 3 * (size_t)h->ld * B), res::want(h->dprow3[1], 3 * (size_t)h->ld * B),
                            res::want(h->dxg, gw), res::want(h->dbg, gw), res::want(h->dsync, (size_t)chain_sync_words()),
                            res::want(h->dpre[0], B), res::want(h->dpre[1], B), res::want(h->dgmu, 128 * B)));
  if (fresh) {
    HIP_TRY(h, hipMemsetAsync(h->dsync.p, 0, sizeof(unsigned) * chain_sync_words(), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // (the second stream's launches read the counters too)
  }
  // the pose rows "before the first cadence": where the previous cadence's panel launch would have left them
  launch_snap_pose(h->stream, bank_view(h), bank_n_hi(h, false), step_bufs(h).prow3_in);
  HIP_TRY(h, hipGetLastError());
  return EKF_OK;
}

// ---- the fused cadences of ekf_stream_run: what is launched, on which stream and in which order is ekf_host_plan.h's
// plan_cadence_launches (the three orders -- serial, look-ahead, chained -- are described there); here the list is executed ----

// one event recorded on `from`, waited for by `to`
static int hand_over(ekf_handle* h, const char* what, Event& ev, hipStream_t from, hipStream_t to) {
  RES_TRY(h, what, ev.record(from));
  HIP_TRY(h, hipStreamWaitEvent(to, ev.ev, 0));
  return EKF_OK;
}
// whatever is still running on the second stream is waited for by the handle's own stream
// (ev_pass: behind the last chained pass, one event per chain of cadences)
static int join_aux(ekf_handle* h) {
  if (!h->run.aux_pass) return EKF_OK;
  if (int rc = hand_over(h, "ev_pass", h->ev_pass, h->aux, h->stream)) return rc;
  h->run.aux_pass = false;
  return EKF_OK;
}

// The innovation log of a cadence solve that used plan `dpl` and wrote `co` (on the handle's stream right behind it: the records
// are read before the next solve into the same copy -- two solves later -- starts).
static void log_cadence(ekf_handle* h, const CadPlan* dpl, const CadOut* co) {
  if (!h->dinnov.p || h->lg_tslot < 0) return;
  launch_innov_cad(h->stream, h->d_stream.p, dpl, co, h->dcfg.enable_measurement_model, h->dcfg.gate_rej != nullptr, h->batch,
                   innov_log(h, h->lg_tslot, 0));
}

// Cadence c of the run in flight (h->run_plan, uploaded).  The optional buffers its plan may want exist before its first launch
// (between the enqueue of a launch that waits on a device-side counter and the enqueue of the launch that advances it the host
// must not block -- an allocation may); then one loop over the planned ops.  A failure before the marked op (no_way_back) has been
// launched returns its error, with CadRun put back to what has in fact been enqueued (the plan advanced it as a whole); once
// it has, the rest of the list is still enqueued, but for the pass -- no device-side wait is left without its counterpart --,
// both streams are synchronised and every trajectory is marked undefined (EKF_ERR_STATE from then on, until it is uploaded again).
static int enqueue_cadence(ekf_handle* h, int c, bool presolved, bool* next_presolved) {
  static const char* const OP_NAME[] = {"solve", "innovation log", "chain", "gate", "panel", "covariance pass", "mark", "gather", "fork", "join",
                                        "join of the second stream"};
  *next_presolved = false;
  const RunPlan& rp = h->run_plan;
  // (the pose log: k_solve_cad_plog writes stream step t's row (pl_tslot + t) % pose_cap itself; nullptr: off)
  const PoseLog plg_on = pose_log(h, h->pl_tslot);
  const PoseLog* plg = h->dpose.p && h->pl_tslot >= 0 ? &plg_on : nullptr;
  const int n_hi = bank_n_hi(h, false);
  const CadPlan* dpl = h->plan2[h->plan_cur].device() + (size_t)c * h->batch;
  const CadPlan* const row[2] = {dpl, dpl + h->batch};
  const BankView bank = bank_view(h);
  for (int b = 0; b < h->batch; ++b) h->neff_enq[b] = rp.entries[(size_t)c * h->batch + b].neff;
  CadStepPlan cp = plan_cadence_step(h, rp, c, n_hi, presolved);
  if (cp.gather_cols && !h->dcolbuf.ensure((size_t)h->batch * CAD_CU * h->ld).ok()) {
    // (an optional optimisation: where its buffer cannot be had the panel launch gathers everything itself, bit-identically)
    (void)hipGetLastError();
    h->opt_col_gather = 0;
    cp = plan_cadence_step(h, rp, c, n_hi, presolved);
  }
  if (cp.beside && !cp.chain_next)                     // (a chained run's set holds it: prepare_piece)
    RES_TRY(h, "the look-ahead's block buffer", h->dgbuf.ensure((size_t)cadence_gbuf_doubles() * h->batch));
  // this cadence's buffers and the next one's, for the solve enqueued ahead (the same copies before and behind the PANEL op's flip)
  const StepBufs bufs[2] = {step_bufs(h, CAD_THIS), step_bufs(h, CAD_NEXT)};
  const CadRun before = h->run;
  const CadLaunches L = plan_cadence_launches(h, rp, c, n_hi, presolved, cp);
  int rc = EKF_OK;
  bool committed = false;                              // the marked op's launch has been attempted
  unsigned done = 0;                                   // op kinds that went out (bit per kind)
  std::string first_err;
  for (int i = 0; i < L.n; ++i) {
    const CadOp& op = L.op[i];
    if (rc != EKF_OK && op.kind == OP_PASS) continue;
    const hipStream_t st = op.stream == ON_AUX ? h->aux : h->stream;
    const StepBufs& s = bufs[op.which];
    int e = EKF_OK;
    switch (op.kind) {
      case OP_SOLVE: {
        SolveCadArgs sx;
        sx.gbuf = op.gparts ? h->dgbuf.p : nullptr, sx.gparts = op.gparts;
        sx.colbuf = op.colbuf ? h->dcolbuf.p : nullptr, sx.col_wgs = op.col_wgs;
        sx.chain = op.chain;
        if (op.sync) sx.gmu = h->dgmu.p, sx.sync = h->dsync.p;
        sx.start_sigma = op.sigma, sx.pre = op.pre_in >= 0 ? h->dpre[op.pre_in].p : nullptr;
        e = launch_profiled(h, op.cls, st, [&] {
          committed = committed || op.no_way_back;
          launch_solve_cad(st, bank, s, h->d_stream.p, row[op.which], h->dcfg, n_hi, sx, plg);
        });
        break;
      }
      case OP_LOG: log_cadence(h, row[op.which], s.cad); break;
      case OP_CHAIN: {
        ChainArgs cx{h->dgbuf.p, h->dgmu.p, h->dxg.p, h->dbg.p, h->dsync.p};
        cx.sigma = op.sigma, cx.gather_target = op.target, cx.gw = op.gw, cx.wait_pass = op.wait_pass;
        cx.pre_in = op.pre_in >= 0 ? h->dpre[op.pre_in].p : nullptr, cx.pre_out = op.pre_out >= 0 ? h->dpre[op.pre_out].p : nullptr;
        cx.plan2 = op.plan2 ? row[op.which] + h->batch : nullptr;
        e = launch_profiled(h, op.cls, st, [&] { launch_chain_cad(st, bank, bufs[CAD_THIS], h->d_stream.p, row[op.which], h->dcfg, cx); });
        break;
      }
      case OP_GATE: launch_gate(st, h->dsync.p, op.sigma, h->dflags.p, h->batch); break;
      case OP_PANEL: {
        PanelCadArgs px{op.nrp, op.form, op.skipw, op.colbuf ? h->dcolbuf.p : nullptr};
        if (op.sync) px.sync = h->dsync.p, px.tail_target = op.target, px.start_sigma = op.sigma;
        StepBufs pb = s;
        if (!op.keep_prow3) pb.prow3_out = nullptr;
        e = launch_profiled(h, op.cls, st, [&] { launch_panels_cad(st, bank, pb, n_hi, px); });
        h->dcur ^= 1;
        h->cur ^= 1;
        h->pending_k += op.ranks;
        h->pending_steps = op.steps_after;
        break;
      }
      case OP_PASS: e = flush_pending(h, st, op.wv ? s.cad : nullptr); break;
      case OP_MARK: launch_mark(st, h->dsync.p, op.sigma); break;
      case OP_GATHER:
        e = launch_profiled(h, op.cls, st, [&] { launch_gather_cad(st, bank, s.dacc_in, h->d_stream.p, row[op.which], op.kb, h->dcfg, h->dgbuf.p); });
        break;
      case OP_FORK: e = hand_over(h, "ev_fork", h->ev_fork, h->stream, h->aux); break;
      case OP_JOIN: e = hand_over(h, "ev_join", h->ev_join, h->aux, h->stream); break;
      case OP_JOIN_AUX: e = hand_over(h, "ev_pass", h->ev_pass, h->aux, h->stream); break;
    }
    // (the launches are checked where the cadence's own kernels go out: a failed log or gate launch shows at the next of them,
    //  the pass and the events' hand-overs check themselves)
    const bool check = op.kind == OP_SOLVE || op.kind == OP_CHAIN || op.kind == OP_PANEL || op.kind == OP_MARK || op.kind == OP_GATHER;
    if (e == EKF_OK && check && hipGetLastError() != hipSuccess)
      e = fail(h, EKF_ERR_HIP, std::string("fused cadence: launch of the ") + OP_NAME[op.kind] + (op.which == CAD_NEXT ? " (next cadence) failed" : " failed"));
    if (e == EKF_OK) {
      done |= 1u << op.kind;
      continue;
    }
    if (!committed) {
      // what the plan advanced and the launches did not: the parity and the cadence's count move with the panel launch, the
      // inputs formed ahead with the chain launch, the second stream stays to be joined unless the join went out; the other
      // statistics count completed cadences.  sigma, gather_count and the serial only grow: they mirror the device's counters.
      CadRun& r = h->run;
      if (!(done & 1u << OP_PANEL)) r.cpar = before.cpar, r.cadences = before.cadences, r.cadence_traj_steps = before.cadence_traj_steps;
      if (!(done & 1u << OP_CHAIN)) r.pre_serial[0] = before.pre_serial[0], r.pre_serial[1] = before.pre_serial[1];
      r.aux_pass = before.aux_pass && !(done & 1u << OP_JOIN_AUX);
      r.lookaheads = before.lookaheads, r.chained = before.chained, r.w_from_v_passes = before.w_from_v_passes;
      return e;
    }
    if (rc == EKF_OK) rc = e, first_err = h->err;
  }
  if (rc != EKF_OK) {
    (void)hipStreamSynchronize(h->aux);
    (void)hipStreamSynchronize(h->stream);
    h->run.aux_pass = false;
    std::fill(h->host_bad.begin(), h->host_bad.end(), (unsigned char)1);
    h->err = first_err;
    return rc;
  }
  *next_presolved = L.next_presolved;
  return EKF_OK;
}

// The input ring (res::InputRing; h_ring / d_ring, h_det / d_det, h_pred / d_pred share its slots).  A call takes a slot, fills
// the pinned records `hs` of it, submits them, launches on *in and reports the launch:
//   staged path: the records are copied to `ds`, which the kernels read;
//   direct path (the small-state path): the one workgroup per trajectory fetches its 352-byte record straight from the pinned
//   ring (one coalesced read over PCIe, ~1.5 us) -- a staged host-to-device copy in front of the kernel costs 5 - 10 us of
//   latency per step, which at these sizes is a third of the step -- and the slot is free once the kernel has run.
constexpr const char* RING_WHAT = "the input ring";
template <class T> struct RingSlot { int slot = 0; T *hs = nullptr, *ds = nullptr; };
template <class T, class H, class D>
static int ring_take(ekf_handle* h, H& host, D& dev, RingSlot<T>* r) {
  RES_TRY(h, RING_WHAT, h->ring.take(h->stream, &r->slot));
  r->hs = host.p + (size_t)r->slot * h->batch;
  r->ds = dev.p + (size_t)r->slot * h->batch;
  return EKF_OK;
}
template <class T>
static int ring_submit(ekf_handle* h, const RingSlot<T>& r, bool direct, size_t count, const T** in) {
  RES_TRY(h, RING_WHAT, h->ring.submit(r.slot, direct, r.ds, r.hs, sizeof(T) * count, h->stream));
  *in = direct ? r.hs : r.ds;
  return EKF_OK;
}
template <class T>
static int ring_launched(ekf_handle* h, const RingSlot<T>& r, bool direct) {
  RES_TRY(h, RING_WHAT, h->ring.launched(r.slot, direct, h->stream));
  return EKF_OK;
}

// While an entry point enqueues `steps` logged steps: the log rows of its launches (ekf_handle::lg_slot, pl_slot).  `innov`: the
// call logs innovations (a lone prediction does not); every call is a row of the pose log.  The counters move in commit() only:
// a call that returns early has logged nothing.  Nothing is logged outside a scope.
struct LogScope {
  ekf_handle* h;
  bool innov, pose;
  int steps;
  LogScope(ekf_handle* h_, bool innov_, int steps_ = 1) : h(h_), innov(innov_ && h_->dinnov.p), pose(h_->dpose.p), steps(steps_) { step(0); }
  void step(int k) {                                   // step k of the call's span
    h->lg_slot = innov ? (long)((h->innov_steps + k) % h->innov_cap) : -1;
    h->lg_jbase = 0;
    h->pl_slot = pose ? (long)((h->pose_steps + k) % h->pose_cap) : -1;
  }
  void pass(int p) { h->lg_jbase = MMAX * p; }         // update pass p of the call's one step: its landmarks from MMAX * p on
  // the span is steps [first, first + steps) of the uploaded stream: its kernels log stream step t in row (lg_tslot + t) % cap
  void stream(int first) {
    const long cap = h->innov_cap, pcap = h->pose_cap;
    if (innov) h->lg_tslot = (long)(((h->innov_steps - first) % cap + cap) % cap);
    if (pose) h->pl_tslot = (long)(((h->pose_steps - first) % pcap + pcap) % pcap);
  }
  void commit() {
    if (innov) h->innov_steps += steps;
    if (pose) h->pose_steps += steps;
  }
  ~LogScope() {
    h->lg_slot = h->lg_tslot = h->pl_slot = h->pl_tslot = -1;
    h->lg_jbase = 0;
  }
};

static int do_step(ekf_handle* h, const char* fn, int base_flags, const double* lin, const double* ang, const int* idx,
                   const double* range, const double* bearing, const int* m, int stride, int fetch_b = -1) {
  if (!h) return EKF_ERR_ARG;
  if (int rc = check_host_bad(h, fn)) return rc;
  if (int rc = refresh_sizes(h)) return rc;
  const bool upd = (base_flags & FLAG_UPDATE) != 0, pred = (base_flags & FLAG_PREDICT) != 0;
  ObsPlan op;                                            // everything is checked before any handle state changes
  if (const char* why = plan_obs_lists(h, pred, upd, true, lin, ang, idx, range, bearing, m, stride, op)) return bad_arg(h, fn, why);
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = push_floor(h, false)) return rc;
  LogScope log(h, upd);
  for (int p = 0; p < op.passes; ++p) {
    log.pass(p);
    const bool direct = small_path(h);
    RingSlot<StepIn> r;
    if (int rc = ring_take(h, h->h_ring, h->d_ring, &r)) return rc;
    const int m_pass_hi = fill_step_records(h, pred, upd, lin, ang, idx, range, bearing, m, stride, p, r.hs);
    h->fetch_b = p == op.passes - 1 ? fetch_b : -1;
    const StepIn* in;
    if (int rc = ring_submit(h, r, direct, (size_t)h->batch, &in)) return rc;
    if (int rc = enqueue_pass(h, in, m_pass_hi)) return rc;
    if (int rc = ring_launched(h, r, direct)) return rc;
  }
  h->fetch_b = -1;
  if (int rc = log_pose_step(h)) return rc;
  log.commit();
  return EKF_OK;
}

// ---- device-side association ------------------------------------------------------------------
static int assoc_init(ekf_handle* h) {
  const size_t B = (size_t)h->batch;
  auto with_group = [&](auto f) {
    return f(res::want(h->dtagmap, TAGMAX * B), res::want(h->dneff, B), res::want(h->d_det, B * RING), res::want(h->h_det, B * RING),
             res::want(h->d_assoc_step, B * 2),         // two update passes: the first 16 landmarks, the rest
             res::want(h->d_assoc_out, B));
  };
  if (with_group([](auto... m) { return res::complete(m...); })) return EKF_OK;   // (every window comes through here)
  HIP_TRY(h, hipSetDevice(h->device));
  bool fresh;
  RES_TRY(h, "the device-side association's buffers", with_group([&](auto... m) { return res::ensure_group(&fresh, m...); }));
  if (fresh) {
    HIP_TRY(h, hipMemsetAsync(h->dtagmap.p, 0xFF, sizeof(int) * TAGMAX * h->batch, h->stream));   // -1
    HIP_TRY(h, hipMemsetAsync(h->d_assoc_out.p, 0, sizeof(AssocOut) * h->batch, h->stream));
  }
  return EKF_OK;
}

// One window per trajectory through the ring (staged on every path), for both detection entries; *in: the device's records.
static int upload_detections(ekf_handle* h, const double* lin, const double* ang, const int* count, const int* tag_id,
                             const double* pose_t, const double* pose_err, int stride, const DetIn** in) {
  RingSlot<DetIn> r;
  if (int rc = ring_take(h, h->h_det, h->d_det, &r)) return rc;
  fill_det_records(h, lin, ang, count, tag_id, pose_t, pose_err, stride, r.hs);
  // the host's view of the active bound must be on the device before the first device-side window
  if (!h->sizes_dirty)
    HIP_TRY(h, hipMemcpyAsync(h->dneff.p, h->neff.data(), sizeof(int) * h->batch, hipMemcpyHostToDevice, h->stream));
  return ring_submit(h, r, false, (size_t)h->batch, in);
}

extern "C" int ekf_set_association(ekf_handle* h, double gate_range, const int* ignore_tags, int n_ignore) {
  if (!h) return EKF_ERR_ARG;
  if (n_ignore < 0 || n_ignore > IGNMAX || (n_ignore > 0 && !ignore_tags))
    return fail(h, EKF_ERR_ARG, "ekf_set_association: at most 16 ignored tags");
  h->acfg.gate2 = gate_range * gate_range;
  h->acfg.n_ignore = n_ignore;
  for (int i = 0; i < n_ignore; ++i) h->acfg.ignore[i] = ignore_tags[i];
  return EKF_OK;
}

extern "C" int ekf_step_detections(ekf_handle* h, const double* lin, const double* ang, const int* count,
                                   const int* tag_id, const double* pose_t, const double* pose_err, int stride) {
  const char* fn = "ekf_step_detections";
  if (!h) return EKF_ERR_ARG;
  if (int rc = check_host_bad(h, fn)) return rc;
  // (checked before anything is allocated, pushed or taken; m_hi, an upper bound of the landmarks observed this window, selects
  //  the kernel instantiation)
  int m_hi = 0;
  if (const char* why = plan_det_windows(h, lin, ang, count, tag_id, pose_t, pose_err, stride, &m_hi)) return bad_arg(h, fn, why);
  if (int rc = assoc_init(h)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = push_floor(h, false)) return rc;
  const DetIn* ds;
  if (int rc = upload_detections(h, lin, ang, count, tag_id, pose_t, pose_err, stride, &ds)) return rc;
  LogScope log(h, true);
  const int mcap = cap_for(std::min(m_hi, MMAX));
  if (((h->pending_k + ranks_for(mcap) + 3) & ~3) > KTOT)   // (what the step's kernels will write: see enqueue_pass)
    if (int rc = flush_pending(h)) return rc;
  h->acfg.active_bound = h->opt_active_bound;
  launch_associate(h->stream, bank_view(h), ds, h->dtagmap.p, h->dneff.p, h->dmu2[h->cur].p, h->d_assoc_step.p, h->d_assoc_out.p, h->acfg,
                   h->n_max, h->pending_k);
  HIP_TRY(h, hipGetLastError());
  h->sizes_dirty = true;
  // m_hi == 0 only when no trajectory has a detection (or the measurement model is off): then, with nothing
  // pending, the O(n) prediction-only kernel applies; any detection selects the generic path, which is also
  // right when the gate leaves nothing (its ranks are zero)
  // (more than EKF_MMAX distinct tags in some trajectory's window: a second pass with the rest -- an update without a
  //  prediction; trajectories that had fewer find m = 0 there)
  if (int rc = enqueue_pass(h, h->d_assoc_step.p, std::min(m_hi, MMAX))) return rc;
  log.pass(1);
  if (m_hi > MMAX)
    if (int rc = enqueue_pass(h, h->d_assoc_step.p + h->batch, m_hi - MMAX)) return rc;
  if (int rc = log_pose_step(h)) return rc;
  log.commit();
  return EKF_OK;
}

extern "C" int ekf_download_tags(ekf_handle* h, int b, int* m, int* idx, int* tag_id, double* xw, double* yw,
                                 double* err, double* range, double* bearing) {
  if (int rc = check_b(h, b, "ekf_download_tags")) return rc;
  if (!h->d_assoc_out.p) return fail(h, EKF_ERR_STATE, "ekf_download_tags: no device-side association has run");
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_internal(h, b, "ekf_download_tags")) return rc;
  AssocOut a;
  HIP_TRY(h, hipMemcpyAsync(&a, h->d_assoc_out.p + b, sizeof(a), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (m) *m = a.m;
  for (int i = 0; i < AMAX; ++i) {
    if (idx) idx[i] = a.idx[i];
    if (tag_id) tag_id[i] = a.tag_id[i];
    if (xw) xw[i] = a.xw[i];
    if (yw) yw[i] = a.yw[i];
    if (err) err[i] = a.err[i];
    if (range) range[i] = a.range[i];
    if (bearing) bearing[i] = a.bearing[i];
  }
  return EKF_OK;
}

extern "C" int ekf_download_tag_index(ekf_handle* h, int b, int* tag_of_index, int capacity, int* n_landmarks) {
  if (int rc = check_b(h, b, "ekf_download_tag_index")) return rc;
  if (!n_landmarks) return fail(h, EKF_ERR_ARG, "ekf_download_tag_index: NULL");
  if (int rc = assoc_init(h)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_internal(h, b, "ekf_download_tag_index")) return rc;
  std::vector<int> tm(TAGMAX);
  HIP_TRY(h, hipMemcpyAsync(tm.data(), h->dtagmap.p + (size_t)b * TAGMAX, sizeof(int) * TAGMAX, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  int count = 0;
  for (int id = 0; id < TAGMAX; ++id)
    if (tm[id] >= 0) {
      count = std::max(count, tm[id] + 1);
      if (tag_of_index && tm[id] < capacity) tag_of_index[tm[id]] = id;
    }
  *n_landmarks = count;
  return EKF_OK;
}

extern "C" int ekf_upload_tag_index(ekf_handle* h, int b, const int* tag_of_index, int n_landmarks) {
  if (int rc = check_b(h, b, "ekf_upload_tag_index")) return rc;
  if (n_landmarks < 0 || (n_landmarks > 0 && !tag_of_index)) return fail(h, EKF_ERR_ARG, "ekf_upload_tag_index: bad arguments");
  if (int rc = assoc_init(h)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<int> tm(TAGMAX, -1);
  for (int i = 0; i < n_landmarks; ++i) {
    if (tag_of_index[i] < 0 || tag_of_index[i] >= TAGMAX) return fail(h, EKF_ERR_ARG, "ekf_upload_tag_index: tag id outside [0, 1024)");
    tm[tag_of_index[i]] = i;
  }
  HIP_TRY(h, hipMemcpyAsync(h->dtagmap.p + (size_t)b * TAGMAX, tm.data(), sizeof(int) * TAGMAX, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

// ---- the two-handle calls (ekf_copy_trajectories, ekf_join_maps) ----
// Each is pair_begin, its plan function (the sizes of both handles are current), pair_flags, pair_defined for every trajectory
// it names, pair_flush, then its tables and its launch on the destination's stream.  Every error is the destination's; what fails inside the source is reworded "`fn`: source: ...".
static int pair_source_fail(ekf_handle* dst, ekf_handle* src, const char* fn, int rc) {
  return src == dst ? rc : fail(dst, rc, std::string(fn) + ": source: " + src->err);
}
static int pair_begin(ekf_handle* dst, ekf_handle* src, const char* fn) {
  if (!dst || !src) return EKF_ERR_ARG;
  if (int rc = refresh_sizes(src)) return pair_source_fail(dst, src, fn, rc);
  return refresh_sizes(dst);
}
// trajectory t of `h`, `which` ("source" / "destination") of the call, must be defined (its flags have been read back)
static int pair_defined(ekf_handle* dst, const char* fn, const ekf_handle* h, const char* which, int t) {
  if (!h->host_bad[t] && !(h->h_flags.p[t] & EKF_FLAG_INTERNAL)) return EKF_OK;
  return fail(dst, EKF_ERR_STATE, std::string(fn) + ": " + which + " trajectory " + std::to_string(t) +
                                      " is undefined (EKF_FLAG_INTERNAL, or an earlier call failed half way): upload it again");
}
// Behind the plan: the source's flags, behind everything enqueued on its stream, and the destination's where the call reads
// its destinations (a join does, a copy overwrites them).  The call's pair_defined checks follow, then pair_flush.
static int pair_flags(ekf_handle* dst, ekf_handle* src, bool reads_dst) {
  HIP_TRY(dst, hipSetDevice(dst->device));
  HIP_TRY(dst, hipMemcpyAsync(src->h_flags.p, src->dflags.p, sizeof(unsigned) * src->batch, hipMemcpyDeviceToHost, src->stream));
  HIP_TRY(dst, hipStreamSynchronize(src->stream));
  if (reads_dst && src != dst) {
    HIP_TRY(dst, hipMemcpyAsync(dst->h_flags.p, dst->dflags.p, sizeof(unsigned) * dst->batch, hipMemcpyDeviceToHost, dst->stream));
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
  }
  return EKF_OK;
}
// what is pending on either handle applied, and the source's streams idle
static int pair_flush(ekf_handle* dst, ekf_handle* src, const char* fn) {
  if (int rc = flush_pending(src)) return pair_source_fail(dst, src, fn, rc);
  if (src != dst)
    if (int rc = flush_pending(dst)) return rc;
  HIP_TRY(dst, hipStreamSynchronize(src->stream));
  if (src->aux) HIP_TRY(dst, hipStreamSynchronize(src->aux));
  return EKF_OK;
}

// Copy whole filter states between trajectories, on the device (k_copy_traj, ekf_copy.hip): src_b[i] of `src` -> dst_b[i] of
// `dst`.  What is pending on either handle is applied first, then stored values only move: the stored upper triangle, the mean
// (dmu2[cur] of each side), the size word and the sticky flags in ONE launch on the destination's stream, the tag table row and
// the last window's AssocOut by two small copies behind it, the host's mirrors (n, neff, neff_enq, the floor) here.
// The rest of what a handle holds per trajectory, one by one -- each is either a property of the SLOT (kept) or dead once
// nothing is pending (flush_pending has run on both handles, and every ekf_stream_run has joined its second stream):
//   dV, dW, dfac, dso      the pending ranks, their restriction to the gathered indices and the last solve's records: read by the
//                          panel launch and the pass of the step that wrote them; with pending_k = 0 the next solve starts at rank
//                          0 and rewrites what it reads.  neff_enq (what dso[b].neff holds for the planner) is set to the bound.
//   ddacc2                 pending pose-block noise: taken as zero while no rank is pending (flush_pending), then rewritten.
//   dready, dmbox          a single-launch step's completion word and mailbox: compared with the HANDLE's step_seq, which goes
//                          on counting; written and consumed inside one launch.
//   dcad2, dcolbuf         a cadence's records and gathered columns: consumed by its own panel launch and pass.
//   dprow3                 pose rows behind a chained cadence: every chained run starts by taking them from P_base (launch_snap_pose).
//   dgmu, dgbuf, dxg, dbg  the next cadence's block and mean, formed inside a run for its next solve; a run's last cadence forms none.
//   dpre, run.pre_serial   inputs formed one cadence ahead: looked up by the handle's cadence serial (CadRun::cad_serial), which
//                          only grows, and never formed beyond the run's last cadence.
//   dsync, dqueue, drm_flag, rm_seq, step_seq, and CadRun's sigma and gather_count (h->run)   counters of the handle, not of a
//                          trajectory; the rest of CadRun is parities, serials and statistics of the handle too: a copy or a join
//                          leaves the whole struct alone.
//   dfloor                 uploaded from the host's bound by push_floor below.
//   dneff                  the device's copy of the bound: written from the host's before the next device-side window (the sizes
//                          of both handles are refreshed first, so the host's are current).
//   noise, dgate, dinnov, dinnov_m, dpose, d_stream and its host tables   the slot's noise row, gate counter, log rows and
//                          uploaded inputs: NOT copied.  ekf_stream_run's stream_maxlm check decides whether the destination's
//                          uploaded stream still fits; stream_stale is not set.
// A source under EKF_FLAG_INTERNAL or host_bad is refused and a destination in that condition becomes good again -- the
// conditions check_internal / clear_internal test and clear for ekf_upload_state; here the kernel overwrites the flag word.
extern "C" int ekf_copy_trajectories(ekf_handle* dst, const int* dst_b, ekf_handle* src, const int* src_b, int k) {
  const char* fn = "ekf_copy_trajectories";
  if (int rc = pair_begin(dst, src, fn)) return rc;
  CopyPlan cp;
  if (const char* why = plan_copy(dst, dst_b, src, src_b, k, cp)) return fail(dst, EKF_ERR_ARG, why);
  if (k == 0) return EKF_OK;
  if (int rc = pair_flags(dst, src, false)) return rc;
  for (int g = 0; g < cp.groups; ++g)
    if (int rc = pair_defined(dst, fn, src, "source", cp.tab[(size_t)COPY_GROUP_WORDS * g])) return rc;
  if (int rc = pair_flush(dst, src, fn)) return rc;
  RES_TRY(dst, "ekf_copy_trajectories's table", dst->dcp_tab.reserve(cp.tab.size(), (size_t)(COPY_GROUP_WORDS + 1) * dst->batch, dst->stream));
  HIP_TRY(dst, hipMemcpyAsync(dst->dcp_tab.p, cp.tab.data(), sizeof(int) * cp.tab.size(), hipMemcpyHostToDevice, dst->stream));
  // (nontemporal stores unless EKFSLAM_HIP_COPY_NT=0: tools/copy_trajectories_time.py measures both, profiles/copy_trajectories.txt)
  bool nt = true;
  if (const char* e = std::getenv("EKFSLAM_HIP_COPY_NT")) nt = std::atoi(e) != 0;
  launch_copy_traj(dst->stream, nt, bank_view(src), bank_view(dst), src->dmu2[src->cur].p, dst->dmu2[dst->cur].p, dst->dcp_tab.p,
                   cp.groups, cp.n_hi);
  HIP_TRY(dst, hipGetLastError());
  // the device tag table and the last window's tags: the source's, or "no window yet" where the source has never had one
  if (src->dtagmap.p)
    if (int rc = assoc_init(dst)) return rc;
  for (int g = 0; g < cp.groups; ++g) {
    const int* head = cp.tab.data() + (size_t)COPY_GROUP_WORDS * g;
    const int s = head[0];
    for (int q = 0; q < head[2]; ++q) {
      const int d = cp.tab[(size_t)COPY_GROUP_WORDS * cp.groups + head[1] + q];
      if (src->dtagmap.p) {
        HIP_TRY(dst, hipMemcpyAsync(dst->dtagmap.p + (size_t)d * TAGMAX, src->dtagmap.p + (size_t)s * TAGMAX, sizeof(int) * TAGMAX,
                                    hipMemcpyDeviceToDevice, dst->stream));
        HIP_TRY(dst, hipMemcpyAsync(dst->d_assoc_out.p + d, src->d_assoc_out.p + s, sizeof(AssocOut), hipMemcpyDeviceToDevice, dst->stream));
      } else if (dst->dtagmap.p) {
        HIP_TRY(dst, hipMemsetAsync(dst->dtagmap.p + (size_t)d * TAGMAX, 0xFF, sizeof(int) * TAGMAX, dst->stream));
        HIP_TRY(dst, hipMemsetAsync(dst->d_assoc_out.p + d, 0, sizeof(AssocOut), dst->stream));
      }
      dst->n[d] = src->n[s];
      dst->neff[d] = src->neff[s];
      dst->neff_enq[d] = src->neff[s];
      dst->host_bad[d] = 0;
    }
  }
  if (int rc = push_floor(dst, true)) return rc;
  HIP_TRY(dst, hipStreamSynchronize(dst->stream));
  return EKF_OK;
}

// Append the map of src_b[i] of `src` to trajectory dst_b[i] of `dst`, on the device (k_join, ekf_join.hip; the header has the
// operation).  As ekf_copy_trajectories: what is pending on either handle is applied first, then ONE launch on the destination's
// stream (in sequential mode behind the snapshot of the destinations' pose rows) writes the new columns, the new means and the
// size words -- and, in sequential mode, the pose, its rows and its block.  The host's mirrors follow here: n, the active bound
// (raised to the new n: the appended landmarks are correlated with everything the pose was), neff_enq, the floor; the device tag
// table's row is merged on the host from the two downloaded rows, as ekf_remove_landmarks renumbers.  Existing indices do not
// move, so the destination's uploaded stream stays runnable and its last window's AssocOut stays; no log row, gate counter, noise
// row or sticky flag changes.  The sources are read only.  Unlike a copy, a join READS its destinations: one under
// EKF_FLAG_INTERNAL or host_bad is refused like a source.
extern "C" int ekf_join_maps(ekf_handle* dst, const int* dst_b, ekf_handle* src, const int* src_b, int k, const double* T,
                             const double* covT, int* first, int* twin, int twin_stride) {
  const char* fn = "ekf_join_maps";
  if (int rc = pair_begin(dst, src, fn)) return rc;
  JoinPlan jp;
  if (const char* why = plan_join(dst, dst_b, src, src_b, k, T, covT, twin != nullptr, twin_stride, jp)) return fail(dst, EKF_ERR_ARG, why);
  if (k == 0) return EKF_OK;
  if (int rc = pair_flags(dst, src, true)) return rc;
  for (int i = 0; i < k; ++i) {
    if (int rc = pair_defined(dst, fn, src, "source", jp.tab[(size_t)JOIN_PAIR_WORDS * i + 1])) return rc;
    if (int rc = pair_defined(dst, fn, dst, "destination", jp.tab[(size_t)JOIN_PAIR_WORDS * i])) return rc;
  }
  if (int rc = pair_flush(dst, src, fn)) return rc;
  const size_t ss = (size_t)join_snap_doubles(dst->ld, jp.seq);
  RES_TRY(dst, "ekf_join_maps's table", dst->djn_tab.reserve(jp.tab.size(), (size_t)JOIN_PAIR_WORDS * dst->batch, dst->stream));
  RES_TRY(dst, "ekf_join_maps's snapshot", dst->djn_snap.reserve(ss * k, ss * k, dst->stream));
  HIP_TRY(dst, hipMemcpyAsync(dst->djn_tab.p, jp.tab.data(), sizeof(int) * jp.tab.size(), hipMemcpyHostToDevice, dst->stream));
  if (!jp.seq)
    HIP_TRY(dst, hipMemcpyAsync(dst->djn_snap.p, jp.frame.data(), sizeof(double) * jp.frame.size(), hipMemcpyHostToDevice, dst->stream));
  if (int rc = launch_profiled(dst, 6, dst->stream, [&] {
        launch_join(dst->stream, bank_view(src), bank_view(dst), src->dmu2[src->cur].p, dst->dmu2[dst->cur].p, dst->djn_tab.p,
                    dst->djn_snap.p, k, jp.tiles_hi, jp.na_hi, jp.seq);
      }))
    return rc;
  HIP_TRY(dst, hipGetLastError());
  for (int i = 0; i < k; ++i) {
    const int* w = jp.tab.data() + (size_t)JOIN_PAIR_WORDS * i;
    const int d = w[0], n_new = 3 + 2 * (w[2] + w[3]);
    if (first) first[i] = w[2];
    dst->n[d] = n_new;
    dst->neff[d] = n_new;
    dst->neff_enq[d] = n_new;
  }
  if (twin) std::fill_n(twin, (size_t)k * twin_stride, -1);
  // the device tag table: an appended landmark keeps its tag unless the destination's map holds that tag already (a twin)
  if (src->dtagmap.p && jp.nb_hi > 0) {
    const bool had = dst->dtagmap.p != nullptr;
    if (int rc = assoc_init(dst)) return rc;
    std::vector<int> ts((size_t)TAGMAX), td((size_t)TAGMAX);
    for (int i = 0; i < k; ++i) {
      const int* w = jp.tab.data() + (size_t)JOIN_PAIR_WORDS * i;
      if (w[3] == 0) continue;
      HIP_TRY(dst, hipMemcpyAsync(ts.data(), src->dtagmap.p + (size_t)w[1] * TAGMAX, sizeof(int) * TAGMAX, hipMemcpyDeviceToHost, dst->stream));
      HIP_TRY(dst, hipMemcpyAsync(td.data(), dst->dtagmap.p + (size_t)w[0] * TAGMAX, sizeof(int) * TAGMAX, hipMemcpyDeviceToHost, dst->stream));
      HIP_TRY(dst, hipStreamSynchronize(dst->stream));
      bool changed = false;
      for (int id = 0; id < TAGMAX; ++id) {
        const int j = ts[id];
        if (j < 0 || j >= w[3]) continue;
        if (td[id] >= 0) {
          if (twin && had) twin[(size_t)i * twin_stride + j] = td[id];
        } else {
          td[id] = w[2] + j;
          changed = true;
        }
      }
      if (changed) {
        HIP_TRY(dst, hipMemcpyAsync(dst->dtagmap.p + (size_t)w[0] * TAGMAX, td.data(), sizeof(int) * TAGMAX, hipMemcpyHostToDevice, dst->stream));
        HIP_TRY(dst, hipStreamSynchronize(dst->stream));
      }
    }
  }
  HIP_TRY(dst, hipMemcpyAsync(dst->dn.p, dst->n.data(), sizeof(int) * dst->batch, hipMemcpyHostToDevice, dst->stream));
  if (int rc = push_floor(dst, true)) return rc;
  HIP_TRY(dst, hipStreamSynchronize(dst->stream));
  return EKF_OK;
}

// Move trajectories [b0, b0 + count) into another frame, in place (k_transform, ekf_transform.hip; the header has the operation).
// As ekf_remove_landmarks and ekf_join_maps: what is pending is applied first, the old means go behind the heads of the frame
// heads by one copy on the handle's stream, then ONE launch rewrites the stored triangle and the means.  The host's
// mirrors follow here: with a covariance the active bound becomes the size (every item is correlated with every other), as a
// join raises it -- neff, neff_enq, the floor; without one it stays.  The last window's world positions (AssocOut xw, yw) are
// mapped on the host, as ekf_remove_landmarks renumbers them.  Sizes, the tag table, noise rows, gate counters, sticky flags and
// log rows do not change, and the uploaded stream stays runnable (ranges, bearings and increments are frame-free).
extern "C" int ekf_transform(ekf_handle* h, int b0, int count, const double* T, const double* cov) {
  const char* fn = "ekf_transform";
  if (int rc = check_b(h, 0, fn)) return rc;
  TransformPlan tp;
  if (const char* why = plan_transform(h, b0, count, T, cov, tp)) return bad_arg(h, fn, why);
  if (count == 0) return EKF_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_internal(h, b0, fn)) return rc;    // (the flags of the whole bank are back)
  for (int t = b0 + 1; t < b0 + count; ++t)
    if (h->host_bad[t] || (h->h_flags.p[t] & EKF_FLAG_INTERNAL)) return check_internal(h, t, fn);
  if (int rc = join_aux(h)) return rc;
  if (int rc = flush_pending(h)) return rc;
  if (tp.applied == 0) {                               // T = 0 without a covariance: every trajectory stays bit for bit
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return EKF_OK;
  }
  const size_t fs = (size_t)transform_frame_doubles(h->ld);
  RES_TRY(h, "ekf_transform's table", h->dtf_tab.reserve(tp.tab.size(), (size_t)TF_WORDS * h->batch, h->stream));
  RES_TRY(h, "ekf_transform's frames", h->dtf_frame.reserve(fs * count, fs * count, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->dtf_tab.p, tp.tab.data(), sizeof(int) * tp.tab.size(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->dtf_frame.p, tp.head.data(), sizeof(double) * tp.head.size(), hipMemcpyHostToDevice, h->stream));
  double* mu = h->dmu2[h->cur].p;
  HIP_TRY(h, hipMemcpyAsync(h->dtf_frame.p + (size_t)TF_HEAD * count, mu + (size_t)b0 * h->ld, sizeof(double) * (size_t)h->ld * count,
                            hipMemcpyDeviceToDevice, h->stream));
  // (nontemporal stores unless EKFSLAM_HIP_TRANSFORM_NT=0: tools/transform_time.py measures both, profiles/transform.txt)
  bool nt = true;
  if (const char* e = std::getenv("EKFSLAM_HIP_TRANSFORM_NT")) nt = std::atoi(e) != 0;
  if (int rc = launch_profiled(h, 8, h->stream, [&] { launch_transform(h->stream, nt, bank_view(h), mu, h->dtf_tab.p, h->dtf_frame.p, count, tp.tiles_hi); }))
    return rc;
  HIP_TRY(h, hipGetLastError());
  if (tp.with_cov) {
    for (int t = b0; t < b0 + count; ++t) h->neff[t] = h->neff_enq[t] = h->n[t];
    if (int rc = push_floor(h, true)) return rc;
  }
  // the last window's tags_positions record: world positions through T
  if (h->d_assoc_out.p) {
    std::vector<AssocOut> ao((size_t)count);
    HIP_TRY(h, hipMemcpyAsync(ao.data(), h->d_assoc_out.p + b0, sizeof(AssocOut) * count, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int bi = 0; bi < count; ++bi) {
      if (!tp.tab[(size_t)TF_WORDS * bi + 3]) continue;
      const double* t = T + 3 * (size_t)bi;
      const double c = std::cos(t[2]), s = std::sin(t[2]);
      AssocOut& a = ao[(size_t)bi];
      for (int i = 0; i < std::min(a.m, AMAX); ++i) {
        const double x = a.xw[i], y = a.yw[i];
        a.xw[i] = t[0] + (c * x - s * y);
        a.yw[i] = t[1] + (s * x + c * y);
      }
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_assoc_out.p + b0, ao.data(), sizeof(AssocOut) * count, hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

extern "C" int ekf_predict(ekf_handle* h, const double* lin, const double* ang) {
  return do_step(h, "ekf_predict", FLAG_PREDICT, lin, ang, nullptr, nullptr, nullptr, nullptr, 0);
}

// A prediction with the caller's motion model (k_predict_pose, ekf_predict_linear.hip): enqueued like ekf_predict -- the records go
// up through a ring slot as do_step's, nothing is waited for -- behind everything on the handle's stream and on the second one
// (join_aux).  The kernel works on P_base in place, under the pending ranks where there are any: no covariance pass, and neither
// pending_k / pending_steps nor the bound, the floor or any counter moves; cur / dcur do not flip (the pose mean is written in place).
// The pose log gets the step's row from k_pose_step on either path (the small-state path writes rows only from its own launch).
extern "C" int ekf_predict_linear(ekf_handle* h, int b0, int count, const double* pose, const double* F, const double* Q,
                                  const int* apply) {
  if (!h) return EKF_ERR_ARG;
  if (int rc = check_host_bad(h, "ekf_predict_linear")) return rc;
  if (int rc = refresh_sizes(h)) return rc;
  PredictPlan& pp = h->predict_plan;
  if (const char* why = plan_predict_linear(h, b0, count, pose, F, Q, apply, pp)) return bad_arg(h, "ekf_predict_linear", why);
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t B = (size_t)h->batch;
  RES_TRY(h, "ekf_predict_linear's input ring", res::ensure_group(nullptr, res::want(h->d_pred, B * RING), res::want(h->h_pred, B * RING)));
  if (int rc = join_aux(h)) return rc;
  RingSlot<PredictIn> r;
  if (int rc = ring_take(h, h->h_pred, h->d_pred, &r)) return rc;
  std::copy(pp.rec.begin(), pp.rec.end(), r.hs);
  const bool direct = small_path(h);
  const PredictIn* in;
  if (int rc = ring_submit(h, r, direct, (size_t)count, &in)) return rc;
  if (pp.n_hi > 0) {
    if (int rc = launch_profiled(h, 7, h->stream, [&] { launch_predict_pose(h->stream, pending_view(h, b0, count), h->dP.p, h->dmu2[h->cur].p, in, pp.n_hi); }))
      return rc;
    HIP_TRY(h, hipGetLastError());
  }
  if (int rc = ring_launched(h, r, direct)) return rc;
  LogScope log(h, false);                              // a logged step, as a lone ekf_predict
  if (log.pose) {
    launch_pose_step(h->stream, pending_view(h, 0, h->batch), pose_log(h, h->pl_slot));
    HIP_TRY(h, hipGetLastError());
  }
  log.commit();
  return EKF_OK;
}

extern "C" int ekf_update(ekf_handle* h, const int* idx, const double* range, const double* bearing,
                          const int* m, int stride) {
  return do_step(h, "ekf_update", FLAG_UPDATE, nullptr, nullptr, idx, range, bearing, m, stride);
}

extern "C" int ekf_step(ekf_handle* h, const double* lin, const double* ang, const int* idx,
                        const double* range, const double* bearing, const int* m, int stride) {
  return do_step(h, "ekf_step", FLAG_PREDICT | FLAG_UPDATE, lin, ang, idx, range, bearing, m, stride);
}

// ---- localisation on a frozen map (ekf_localize_step / _update / _run; k_loc_solve + k_loc_rows, ekf_localize.hip) ----
// Every entry is loc_begin -- what runs on the second stream is joined, what is pending is applied by the ordinary pass, once:
// the kernels work on P_base with nothing pending, and leave nothing pending -- then per step (per update pass of a step) loc_pass:
// the two launches in their profile brackets (classes 9 and 10), the innovation log's copy of the solve's y / S^-1 (k_innov_step
// reads them where k_solve leaves its own), and behind a step its pose-log row (k_pose_step, on either path as for
// ekf_predict_linear).  Neither pending_k / pending_steps nor any counter moves and cur / dcur do not flip: the pose mean is
// written in place.  A failure after the first launch leaves every trajectory undefined (host_bad: EKF_ERR_STATE from then on).
static int loc_begin(ekf_handle* h) {
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = join_aux(h)) return rc;
  if (int rc = flush_pending(h)) return rc;
  RES_TRY(h, "the localisation records", h->dloc.reserve((size_t)h->batch, 0, h->stream));
  return EKF_OK;
}
static int loc_pass(ekf_handle* h, const StepIn* in, int groups) {
  const BankView bank = bank_view(h);
  if (int rc = launch_profiled(h, 9, h->stream, [&] { launch_loc_solve(h->stream, bank, h->dmu2[h->cur].p, in, h->dfloor.p, h->dloc.p, h->dcfg); }))
    return rc;
  if (int rc = launch_profiled(h, 10, h->stream, [&] { launch_loc_rows(h->stream, bank, h->dloc.p, groups); })) return rc;
  if (h->dinnov.p && h->lg_slot >= 0)
    launch_innov_step(h->stream, in, h->dso.p, h->dcfg.enable_measurement_model, h->dcfg.gate_rej != nullptr, h->batch,
                      innov_log(h, h->lg_slot, h->lg_jbase));
  HIP_TRY(h, hipGetLastError());
  return EKF_OK;
}
static int loc_pose_row(ekf_handle* h) {
  if (!h->dpose.p || h->pl_slot < 0) return EKF_OK;
  launch_pose_step(h->stream, pending_view(h, 0, h->batch), pose_log(h, h->pl_slot));
  HIP_TRY(h, hipGetLastError());
  return EKF_OK;
}
static int loc_half_failed(ekf_handle* h, int rc) {
  std::fill(h->host_bad.begin(), h->host_bad.end(), (unsigned char)1);
  return rc;
}

static int do_localize(ekf_handle* h, const char* fn, int base_flags, const double* lin, const double* ang, const int* idx,
                       const double* range, const double* bearing, const int* m, int stride) {
  if (!h) return EKF_ERR_ARG;
  if (int rc = check_host_bad(h, fn)) return rc;
  if (int rc = refresh_sizes(h)) return rc;
  const bool upd = (base_flags & FLAG_UPDATE) != 0, pred = (base_flags & FLAG_PREDICT) != 0;
  LocPlan lp;
  if (const char* why = plan_localize(h, pred, upd, lin, ang, idx, range, bearing, m, stride, lp)) return bad_arg(h, fn, why);
  if (int rc = loc_begin(h)) return rc;
  if (int rc = push_floor(h, false)) return rc;
  const bool direct = small_path(h);
  LogScope log(h, upd);
  for (int p = 0; p < lp.passes; ++p) {
    log.pass(p);
    RingSlot<StepIn> r;
    if (int rc = ring_take(h, h->h_ring, h->d_ring, &r)) return p ? loc_half_failed(h, rc) : rc;
    // (the fill raises the host's bound over the pass's landmarks: a general row correlates the pose with the landmark it names)
    fill_step_records(h, pred, upd, lin, ang, idx, range, bearing, m, stride, p, r.hs);
    const StepIn* in;
    if (int rc = ring_submit(h, r, direct, (size_t)h->batch, &in)) return loc_half_failed(h, rc);
    if (int rc = loc_pass(h, in, loc_rows_groups(loc_bound_hi(h)))) return loc_half_failed(h, rc);
    if (int rc = ring_launched(h, r, direct)) return loc_half_failed(h, rc);
  }
  if (int rc = loc_pose_row(h)) return loc_half_failed(h, rc);
  log.commit();
  return EKF_OK;
}

extern "C" int ekf_localize_step(ekf_handle* h, const double* lin, const double* ang, const int* idx, const double* range,
                                 const double* bearing, const int* m, int stride) {
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  return do_localize(h, "ekf_localize_step", FLAG_PREDICT | FLAG_UPDATE, lin, ang, idx, range, bearing, m, stride);
}

extern "C" int ekf_localize_update(ekf_handle* h, const int* idx, const double* range, const double* bearing, const int* m,
                                   int stride) {
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  return do_localize(h, "ekf_localize_update", FLAG_UPDATE, nullptr, nullptr, idx, range, bearing, m, stride);
}

// Steps [first, first + count) of the uploaded stream in localisation mode: the same two launches per step, reading StepIn from
// the stream buffer, back to back without a host synchronisation.  The stream itself is not touched and stays runnable.
extern "C" int ekf_localize_run(ekf_handle* h, int first, int count) {
  const char* fn = "ekf_localize_run";
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_host_bad(h, fn)) return rc;
  if (int rc = refresh_sizes(h)) return rc;
  if (first < 0 || count < 0 || first + count > h->stream_steps)
    return fail(h, EKF_ERR_STATE, "ekf_localize_run: range outside the uploaded stream");
  if (h->stream_stale)
    return fail(h, EKF_ERR_STATE, "ekf_localize_run: landmarks were removed (ekf_remove_landmarks) after the stream was uploaded: its "
                                  "landmark indices and sizes refer to the state before; upload the stream again");
  for (int b = 0; b < h->batch; ++b)                   // the state may have been replaced since the upload
    if (h->stream_maxlm[b] > (h->n[b] - 3) / 2)
      return fail(h, EKF_ERR_STATE, "ekf_localize_run: the uploaded stream observes landmarks the current state does not have");
  if (count == 0) return EKF_OK;
  if (int rc = loc_begin(h)) return rc;
  if (int rc = push_floor(h, true)) return rc;
  LogScope log(h, true, count);
  const int* own_last = h->stream_own.data() + (size_t)(first + count - 1) * h->batch;
  const int groups = loc_rows_groups(loc_bound_hi(h, own_last));
  for (int k = first; k < first + count; ++k) {
    log.step(k - first);
    if (int rc = loc_pass(h, h->d_stream.p + (size_t)k * h->batch, groups)) return loc_half_failed(h, rc);
    if (int rc = loc_pose_row(h)) return loc_half_failed(h, rc);
  }
  log.commit();
  for (int b = 0; b < h->batch; ++b) {
    h->neff[b] = std::max(h->neff[b], std::min(h->n[b], own_last[b]));
    h->neff_enq[b] = h->opt_active_bound ? h->neff[b] : h->n[b];
  }
  return EKF_OK;
}

// One window of raw detections per trajectory in localisation mode: ekf_localize_step on whatever the window matches, with the
// association on the device (k_loc_associate, ekf_loc_assoc.hip) -- no tag table or pose comes back to the host.  What the call
// launches is plan_localize_detections' (ekf_host_plan.h).  loc_begin, the association's buffers, the DetIn records through the
// ring (as ekf_step_detections), k_loc_associate into d_assoc_step / d_assoc_out / d_unmatched, then loc_pass on the first records
// and, where a window may match more than MMAX tags, on the update-only rest; log rows as do_localize writes them.
// The active bound: the device raises dneff over the landmarks it matched and bakes it into the records; the host's mirror
// follows through sizes_dirty (refresh_sizes reads dn -- unchanged: the size never moves -- and dneff back before anything uses
// them; loc_bound_hi, push_floor and the step paths honour the flag as they do behind ekf_step_detections).
extern "C" int ekf_localize_detections(ekf_handle* h, const double* lin, const double* ang, const int* count, const int* tag_id,
                                       const double* pose_t, const double* pose_err, int stride) {
  const char* fn = "ekf_localize_detections";
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_host_bad(h, fn)) return rc;
  LocDetPlan lp;
  if (const char* why = plan_localize_detections(h, lin, ang, count, tag_id, pose_t, pose_err, stride, lp)) return bad_arg(h, fn, why);
  if (int rc = loc_begin(h)) return rc;
  if (int rc = assoc_init(h)) return rc;
  if (!h->d_unmatched.p) {
    RES_TRY(h, "the unmatched-tag records", h->d_unmatched.reserve((size_t)h->batch, 0, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_unmatched.p, 0, sizeof(LocUnmatched) * h->batch, h->stream));
  }
  if (int rc = push_floor(h, false)) return rc;
  const DetIn* ds;
  if (int rc = upload_detections(h, lin, ang, count, tag_id, pose_t, pose_err, stride, &ds)) return rc;
  h->acfg.active_bound = h->opt_active_bound;
  if (int rc = launch_profiled(h, 11, h->stream, [&] {
        launch_loc_associate(h->stream, bank_view(h), ds, h->dtagmap.p, h->dneff.p, h->dmu2[h->cur].p, h->d_assoc_step.p,
                             h->d_assoc_out.p, h->d_unmatched.p, h->acfg);
      }))
    return loc_half_failed(h, rc);
  if (hipGetLastError() != hipSuccess) return loc_half_failed(h, fail(h, EKF_ERR_HIP, std::string(fn) + ": the association's launch failed"));
  h->sizes_dirty = true;
  LogScope log(h, true);
  for (int p = 0; p < lp.passes; ++p) {
    log.pass(p);
    if (int rc = loc_pass(h, h->d_assoc_step.p + (size_t)p * h->batch, lp.groups)) return loc_half_failed(h, rc);
  }
  if (int rc = loc_pose_row(h)) return loc_half_failed(h, rc);
  log.commit();
  return EKF_OK;
}

// The distinct tag ids of trajectory b's last localisation window that its map does not hold, in order of first appearance: *m
// their number, the first min(*m, capacity, EKF_AMAX) of them into tag_id.  Blocking.
extern "C" int ekf_download_unmatched(ekf_handle* h, int b, int* m, int* tag_id, int capacity) {
  const char* fn = "ekf_download_unmatched";
  if (int rc = check_b(h, b, fn)) return rc;
  if (!m || capacity < 0 || (capacity > 0 && !tag_id)) return bad_arg(h, fn, "NULL m, or a capacity without an array");
  if (!h->d_unmatched.p) return fail(h, EKF_ERR_STATE, std::string(fn) + ": no localisation window has run (ekf_localize_detections)");
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = check_internal(h, b, fn)) return rc;
  LocUnmatched u;
  HIP_TRY(h, hipMemcpyAsync(&u, h->d_unmatched.p + b, sizeof(u), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  *m = u.total;
  for (int i = 0; i < std::min(std::min(u.total, AMAX), capacity); ++i) tag_id[i] = u.tag_id[i];
  return EKF_OK;
}

// ekf_step + ekf_download_state(b) in one call: what one iteration of the reference's loop is (EKF_pose_estimation returns
// mean and covariance every call, src/replay_no_ros.py:229-237, :482).  On the small-state path the step's own launch
// leaves trajectory b's state in pinned host memory (k_small_stream's host_out): one launch and one synchronisation per call.
extern "C" int ekf_step_fetch(ekf_handle* h, const double* lin, const double* ang, const int* idx, const double* range,
                              const double* bearing, const int* m, int stride, int b, double* mu, double* P, int n) {
  if (int rc = check_b(h, b, "ekf_step_fetch")) return rc;
  if (!mu || !P) return fail(h, EKF_ERR_ARG, "ekf_step_fetch: NULL output array");
  if (n != h->n[b]) return fail(h, EKF_ERR_ARG, "ekf_step_fetch: n does not match the state size");
  h->fetched = false;
  int want = -1;
  if (n <= PACK_SMALL_N && small_path(h)) {
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = pack_buffer(h)) return rc;
    want = b;
  }
  const int rc_step = do_step(h, "ekf_step_fetch", FLAG_PREDICT | FLAG_UPDATE, lin, ang, idx, range, bearing, m, stride, want);
  h->fetch_b = -1;
  if (rc_step) return rc_step;
  if (!h->fetched) return ekf_download_state(h, b, mu, P, n);
  h->fetched = false;
  h->fused_fetches += 1;
  if (h->opt_fetch_spin) {
    // poll the sequence word the kernel releases behind its stores (pinned, coherent); every few microseconds make sure the
    // stream is still busy -- a launch that failed would otherwise be waited for forever
    const unsigned long long* word = reinterpret_cast<const unsigned long long*>(h->h_pack.p + PACK_WORDS - 1);
    for (long spin = 1;; ++spin) {
      if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == h->fetch_seq) break;
      if ((spin & 4095) == 0) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipErrorNotReady) continue;
        if (q != hipSuccess) return fail(h, EKF_ERR_HIP, std::string("ekf_step_fetch: ") + hipGetErrorString(q));
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == h->fetch_seq) break;
        return fail(h, EKF_ERR_HIP, "ekf_step_fetch: the stream drained without the step's state having been written");
      }
      __builtin_ia32_pause();
    }
    // Integrity: the host has seen the flag word while the launch is still running; that the payload is complete
    // rests on the ordering of the kernel's posted writes (see k_small_stream).  Tripwire: the trailer's copy of the sequence
    // number, written by another wave; with "fetch_verify" also the XOR checksum over the whole payload.  A mismatch falls
    // back to waiting for the launch -- after which every write is visible -- and is counted.
    const unsigned long long* trailer = reinterpret_cast<const unsigned long long*>(h->h_pack.p) + (size_t)n * n + n + 1;
    bool good = __atomic_load_n(trailer, __ATOMIC_ACQUIRE) == h->fetch_seq;
    if (good && h->opt_fetch_verify) {
      const unsigned long long* w = reinterpret_cast<const unsigned long long*>(h->h_pack.p);
      unsigned long long x = 0ull;
      for (size_t i = 0; i < (size_t)n * n + n + 1; ++i) x ^= w[i];
      good = x == trailer[1];
    }
    if (!good) {
      h->fetch_retries += 1;
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
  } else {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  if ((unsigned)h->h_pack.p[(size_t)n * n + n] & EKF_FLAG_INTERNAL) return check_internal(h, b, "ekf_step_fetch");
  std::memcpy(P, h->h_pack.p, sizeof(double) * (size_t)n * n);
  std::memcpy(mu, h->h_pack.p + (size_t)n * n, sizeof(double) * n);
  return EKF_OK;
}

extern "C" int ekf_stream_upload(ekf_handle* h, int steps, const double* lin, const double* ang, const int* idx,
                                 const double* range, const double* bearing, const int* m, int stride) {
  if (!h) return EKF_ERR_ARG;
  if (int rc = refresh_sizes(h)) return rc;
  if (steps <= 0) return fail(h, EKF_ERR_ARG, "ekf_stream_upload: steps must be > 0");
  if (!lin || !ang || !m || stride < 0) return fail(h, EKF_ERR_ARG, "ekf_stream_upload: NULL array");
  if (stride > MMAX) return fail(h, EKF_ERR_ARG, "ekf_stream_upload: stride must be <= EKF_MMAX");
  const size_t count = (size_t)steps * h->batch;
  // validate the whole stream before anything of the previous one is replaced: every count (also with the measurement
  // model off, where a single step's counts are not read), then each step as ekf_step checks a call
  for (size_t e = 0; e < count; ++e)
    if (m[e] < 0 || m[e] > stride) return fail(h, EKF_ERR_ARG, "ekf_stream_upload: m out of range");
  for (int k = 0; k < steps; ++k) {
    const size_t e = (size_t)k * h->batch, o = e * stride;
    ObsPlan op;
    if (const char* why = plan_obs_lists(h, true, true, true, lin + e, ang + e, idx ? idx + o : nullptr, range ? range + o : nullptr,
                                         bearing ? bearing + o : nullptr, m + e, stride, op))
      return bad_arg(h, "ekf_stream_upload", why);
  }
  std::vector<StepIn> host(count);
  h->stream_mhi.assign(steps, 0);
  h->stream_m.assign(count, 0);
  h->stream_own.assign(count, 3);
  h->stream_maxlm.assign(h->batch, 0);
  h->stream_steps = 0;
  // The records carry the bound that follows from the stream's own observations; what the state already
  // correlates when the stream is RUN (possibly later, possibly more than once) is added there (push_floor).
  std::vector<int> own(h->batch, 3);
  for (int k = 0; k < steps; ++k)
    for (int b = 0; b < h->batch; ++b) {
      const size_t e = (size_t)k * h->batch + b;
      const int mb = h->cfg.enable_measurement_model ? m[e] : 0;
      fill_step(host[e], h->n[b], own[b], lin[e], ang[e], FLAG_PREDICT | FLAG_UPDATE, idx ? idx + e * stride : nullptr,
                range ? range + e * stride : nullptr, bearing ? bearing + e * stride : nullptr, mb, 0);
      h->stream_mhi[k] = std::max(h->stream_mhi[k], mb);
      h->stream_m[e] = (unsigned char)host[e].m;
      h->stream_own[e] = own[b];
      for (int i = 0; i < mb; ++i) h->stream_maxlm[b] = std::max(h->stream_maxlm[b], host[e].idx[i] + 1);
    }
  HIP_TRY(h, hipSetDevice(h->device));
  RES_TRY(h, "the uploaded stream", h->d_stream.reserve(count, 0, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_stream.p, host.data(), sizeof(StepIn) * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));      // inputs are resident in HBM from here on
  h->stream_steps = steps;
  h->stream_stale = false;
  return EKF_OK;
}

extern "C" int ekf_stream_run(ekf_handle* h, int first, int count) {
  if (!h) return EKF_ERR_ARG;
  if (int rc = check_host_bad(h, "ekf_stream_run")) return rc;
  if (int rc = refresh_sizes(h)) return rc;
  if (first < 0 || count < 0 || first + count > h->stream_steps)
    return fail(h, EKF_ERR_STATE, "ekf_stream_run: range outside the uploaded stream");
  if (h->stream_stale)
    return fail(h, EKF_ERR_STATE, "ekf_stream_run: landmarks were removed (ekf_remove_landmarks) after the stream was uploaded: its "
                                  "landmark indices and sizes refer to the state before; upload the stream again");
  for (int b = 0; b < h->batch; ++b)                   // the state may have been replaced since the upload
    if (h->stream_maxlm[b] > (h->n[b] - 3) / 2)
      return fail(h, EKF_ERR_STATE, "ekf_stream_run: the uploaded stream observes landmarks the current state does not have");
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = push_floor(h, true)) return rc;
  LogScope log(h, true, count);
  log.stream(first);
  if (small_path(h) && count > 0) {
    // the whole range as ONE launch (in pieces of 4096 steps: a bounded kernel), P resident in LDS across all its steps
    for (int k = first; k < first + count; k += 4096) {
      log.step(k - first);
      if (int rc = enqueue_small(h, h->d_stream.p + (size_t)k * h->batch, std::min(4096, first + count - k))) return rc;
    }
    for (int b = 0; b < h->batch; ++b)
      h->neff[b] = std::max(h->neff[b], std::min(h->n[b], h->stream_own[(size_t)(first + count - 1) * h->batch + b]));
    h->neff_enq = h->neff;
    log.commit();
    return EKF_OK;
  }
  for (int k = first; k < first + count;) {
    // Where nothing is pending the rest of the range runs as packed cadences (ekf_cadence.hip): per cadence one solve launch
    // and one panel launch for a trajectory's next 40 landmark updates and every prediction in between, each trajectory on
    // its own cursor, a covariance pass between two cadences.  While ranks are pending (steps enqueued before this call) the
    // per-step kernels append to them until their pass is due.
    if (cadences_possible(h)) {
      // (planned and uploaded in pieces of at most 8192 steps: 32 B per cadence and trajectory; a piece ends with every
      //  trajectory at its last step, and what its last cadence left pending is flushed so that the next piece starts fused)
      const int piece_end = std::min(first + count, k + 8192);
      plan_cadences(h, k, piece_end, h->run_plan);
      if (int rc = upload_run_plan(h)) return rc;
      if (int rc = prepare_piece(h)) return rc;
      bool presolved = false;                          // the next cadence's solve has been enqueued already (chained / look-ahead)
      for (int c = 0; c < h->run_plan.ncad; ++c)
        if (int rc = enqueue_cadence(h, c, presolved, &presolved)) return rc;
      if (int rc = join_aux(h)) return rc;
      k = piece_end;
      if (k < first + count)
        if (int rc = flush_pending(h)) return rc;
      continue;
    }
    for (int b = 0; b < h->batch; ++b)
      h->neff_enq[b] = std::min(h->n[b], std::max(h->floor_host[b], h->stream_own[(size_t)k * h->batch + b]));
    log.step(k - first);
    if (int rc = enqueue_pass(h, h->d_stream.p + (size_t)k * h->batch, h->stream_mhi[k])) return rc;
    if (int rc = log_pose_step(h)) return rc;
    ++k;
  }
  log.commit();
  if (count > 0)
    for (int b = 0; b < h->batch; ++b)
      h->neff[b] = std::max(h->neff[b], std::min(h->n[b], h->stream_own[(size_t)(first + count - 1) * h->batch + b]));
  // A cadence only forms where nothing is pending (its panel is gathered from P_base alone).  A run's last cadence leaves its
  // ranks pending unless its slots are used up -- right for one long run and for online steps behind it, but a caller that
  // drives the stream in SHORT pieces would alternate between one short cadence and the per-step kernels: "run_end_flush" = 1
  // applies them here (one covariance pass per call) and every piece runs fused.
  if (h->opt_run_end_flush && h->opt_fused_cadence)
    if (int rc = flush_pending(h)) return rc;
  return EKF_OK;
}

extern "C" int ekf_run_stream(ekf_handle* h, int steps, const double* lin, const double* ang, const int* idx,
                              const double* range, const double* bearing, const int* m, int stride) {
  if (!h) return EKF_ERR_ARG;
  if (steps <= 0) return EKF_OK;
  if (int rc = ekf_stream_upload(h, steps, lin, ang, idx, range, bearing, m, stride)) return rc;
  return ekf_stream_run(h, 0, steps);
}

extern "C" int ekf_predict_dense(ekf_handle* h, int b, const double* F, const double* Q) {
  if (int rc = check_b(h, b, "ekf_predict_dense")) return rc;
  if (!F || !Q) return fail(h, EKF_ERR_ARG, "ekf_predict_dense: NULL matrix");
  const int n = h->n[b];
  const size_t bytes = sizeof(double) * (size_t)h->rows * h->ld;
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = materialize(h, b)) return rc;           // the product needs the full matrix
  const size_t words = (size_t)h->rows * h->ld;
  RES_TRY(h, "the dense product's operands",
          res::ensure_group(nullptr, res::want(h->dF, words), res::want(h->dQ, words), res::want(h->dTmp, words)));
  HIP_TRY(h, hipMemsetAsync(h->dF.p, 0, bytes, h->stream));
  HIP_TRY(h, hipMemcpy2DAsync(h->dF.p, sizeof(double) * h->ld, F, sizeof(double) * n, sizeof(double) * n, n,
                              hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpy2DAsync(h->dQ.p, sizeof(double) * h->ld, Q, sizeof(double) * n, sizeof(double) * n, n,
                              hipMemcpyHostToDevice, h->stream));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->profile) {
    if (int rc = prof_event(h, &e0)) return rc;
    if (int rc = prof_event(h, &e1)) return rc;
    HIP_TRY(h, hipEventRecord(e0, h->stream));
  }
  h->neff[b] = n;                                      // a general F correlates everything
  // the product works on plain row-major matrices: a covariance kept in column panels (ld > 4096) goes through a
  // row-major copy (device to device, one 2-D copy per panel each way; 4 n^3 flop dwarf it)
  double* Pdense = h->dP.p + (size_t)b * h->pstride;
  if (p_panels(h->ld) > 1) {
    RES_TRY(h, "the dense product's row-major staging", h->dPlin.ensure(words));
    HIP_TRY(h, copy_cov(h, b, h->dPlin.p, h->ld, 0, 0, n, n, false, true));
    Pdense = h->dPlin.p;
  }
  if (dense_propagate(h->stream, Pdense, h->dTmp.p, h->dF.p, h->dQ.p, n, h->ld) != 0)
    return fail(h, EKF_ERR_HIP, "ekf_predict_dense: launch failed");
  if (p_panels(h->ld) > 1) HIP_TRY(h, copy_cov(h, b, h->dPlin.p, h->ld, 0, 0, n, n, true, true));
  if (h->profile) HIP_TRY(h, hipEventRecord(e1, h->stream));
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

extern "C" int ekf_flush(ekf_handle* h) {
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  return flush_pending(h);
}

extern "C" int ekf_sync(ekf_handle* h) {
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  return check_internal(h, -1, "ekf_sync");          // (synchronises)
}

extern "C" int ekf_status_flags(ekf_handle* h, int b, unsigned* flags) {
  if (int rc = check_b(h, b, "ekf_status_flags")) return rc;
  if (!flags) return fail(h, EKF_ERR_ARG, "ekf_status_flags: NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(flags, h->dflags.p + b, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

extern "C" int ekf_timer_begin(ekf_handle* h) {
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  RES_TRY(h, "t0", h->t0.record(h->stream));
  return EKF_OK;
}

extern "C" int ekf_timer_end(ekf_handle* h, double* elapsed_ms) {
  if (!h || !elapsed_ms) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  RES_TRY(h, "t1", h->t1.record(h->stream));
  RES_TRY(h, "t1", h->t1.wait_if_recorded());
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->t0.ev, h->t1.ev));
  *elapsed_ms = ms;
  return EKF_OK;
}

extern "C" int ekf_profile_enable(ekf_handle* h, int on) {
  if (!h) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->profile = on != 0;
  h->prof_used = 0;
  h->prof_seen = 0;
  // (the events a run will use exist before it starts: creating one inside the run costs the host tens of microseconds)
  if (h->profile)
    while (h->prof_pool.size() < (h->opt_profile_kernels ? 1024u : 128u)) {
      Event e;
      RES_TRY(h, "a profiling event", e.ensure(true));
      h->prof_pool.push_back(std::move(e));
    }
  return EKF_OK;
}

extern "C" int ekf_profile_read(ekf_handle* h, double* pass_ms_total, long long* pass_launches) {
  if (!h || !pass_ms_total || !pass_launches) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (h->aux) HIP_TRY(h, hipStreamSynchronize(h->aux));
  double total = 0.0;
  long long count = 0;
  for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
    if (h->prof_cls[i / 2] != 0) continue;
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->prof_pool[i].ev, h->prof_pool[i + 1].ev));
    total += ms;
    count += 1;
  }
  *pass_ms_total = total;
  *pass_launches = count;
  h->prof_used = 0;
  return EKF_OK;
}

// ("profile_kernels" = 1) the same for the cadence's other launches: cls 1 the solve launch, 2 the chain / look-ahead gather
// launch, 3 the panel launch (0: the covariance pass), 4 k_direct, 5 k_linear, 6 k_join (with its snapshot launch), 7
// k_predict_pose, 8 k_transform, 9 k_loc_solve, 10 k_loc_rows; does not reset -- read these BEFORE ekf_profile_read
extern "C" int ekf_profile_read_class(ekf_handle* h, int cls, double* ms_total, long long* launches) {
  if (!h || !ms_total || !launches) return EKF_ERR_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (h->aux) HIP_TRY(h, hipStreamSynchronize(h->aux));
  double total = 0.0;
  long long count = 0;
  for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
    if (h->prof_cls[i / 2] != cls) continue;
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->prof_pool[i].ev, h->prof_pool[i + 1].ev));
    total += ms;
    count += 1;
  }
  *ms_total = total;
  *launches = count;
  return EKF_OK;
}

extern "C" long long ekf_profile_passes(ekf_handle* h) { return h ? (long long)h->prof_seen : -1; }

// (diagnostics section of the header; no device needed) the equal static shares of the row-slab pass for a
// few long trajectories: out = workgroups x 16 pieces x (trajectory, slab, first strip, strips); returns the pieces of
// the longest share (0: no table) -- tests/test_cpu_host.py checks that every strip of every slab is covered exactly once
extern "C" int ekf_debug_pass_shares(int batch, int n_hi, int workgroups, int* out) {
  if (batch < 1 || n_hi < 3 || workgroups < 1 || !out) return -1;
  return build_pass_shares(batch, n_hi, workgroups, out);
}

// (diagnostics section of the header) pieces of the longest share if the last covariance pass ran on equal
// static shares, else 0
extern "C" int ekf_debug_last_pass_shares(ekf_handle* h) { return h ? h->last_shares : -1; }

// (diagnostics section of the header) how many fused cadences ekf_stream_run has launched and how many steps
// they covered: tests assert that the path they mean to check is the one that ran
extern "C" int ekf_debug_cadences(ekf_handle* h, long* cadences, long* steps) {
  if (!h) return EKF_ERR_ARG;
  if (cadences) *cadences = h->run.cadences;
  if (steps) *steps = h->run.cadence_traj_steps / std::max(h->batch, 1);
  return EKF_OK;
}
// (diagnostics section of the header) how many of them had their solve run beside the previous covariance pass
extern "C" long ekf_debug_lookaheads(ekf_handle* h) { return h ? h->run.lookaheads : -1; }
// (diagnostics section of the header) host fallbacks of the device-side association, as the binding reported them
extern "C" long ekf_debug_assoc_fallbacks(ekf_handle* h) { return h ? h->assoc_fallbacks : -1; }
extern "C" void ekf_debug_note_assoc_fallback(ekf_handle* h) { if (h) h->assoc_fallbacks += 1; }
// (diagnostics section of the header) ... and how many of those had their block formed by k_chain_cad (chained solves)
extern "C" long ekf_debug_chained(ekf_handle* h) { return h ? h->run.chained : -1; }
// ... and covariance passes that formed their W fragments from V and the records ("w_from_v")
extern "C" long ekf_debug_w_from_v(ekf_handle* h) { return h ? h->run.w_from_v_passes : -1; }
extern "C" int ekf_debug_last_pass_wv(ekf_handle* h) { return h ? h->last_wv : -1; }
// (diagnostics section of the header) launches of the small-state path so far
extern "C" long ekf_debug_small_launches(ekf_handle* h) { return h ? h->small_launches : -1; }
extern "C" long ekf_debug_fused_fetches(ekf_handle* h) { return h ? h->fused_fetches : -1; }
extern "C" long ekf_debug_dense_packs(ekf_handle* h) { return h ? h->dense_packs : -1; }
extern "C" long ekf_debug_fetch_retries(ekf_handle* h) { return h ? h->fetch_retries : -1; }

// (diagnostics section of the header) the fused cadence's record of trajectory b (head + per-landmark records)
extern "C" long ekf_debug_cad(ekf_handle* h, int b, void* dst, long bytes) {
  if (!h || b < 0 || b >= h->batch || !h->dcad2[h->run.cpar ^ 1].p) return -1;
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
  const long have = (long)sizeof(CadOut);
  if (dst && bytes > 0 && hipMemcpy(dst, h->dcad2[h->run.cpar ^ 1].p + b, (size_t)std::min(bytes, have), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return have;
}

// (diagnostics section of the header) raw device buffers of trajectory b, exactly as they stand -- no flush,
// no mirror, no status check: which = 0 P_base (device layout, ekf_device.h: rows x ld up to ld = 4096, column panels beyond), 1 V (80 x ld), 2 W (80 x ld, MFMA-tiled), 3 the mean buffer
// the NEXT step reads, 4 the other mean buffer.  Returns the number of doubles the buffer holds (copies min(count, that)).
extern "C" long ekf_debug_snapshot(ekf_handle* h, int b, int which, double* dst, long count) {
  if (!h || b < 0 || b >= h->batch || which < 0 || which > 6) return -1;
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
  const double* src = nullptr;
  long have = 0;
  switch (which) {
    case 0: src = h->dP.p + (size_t)b * h->pstride; have = h->pstride; break;
    case 1: src = h->dV.p + (size_t)b * KTOT * h->ld; have = (long)KTOT * h->ld; break;
    case 2: src = h->dW.p + (size_t)b * KTOT * h->ld; have = (long)KTOT * h->ld; break;
    case 3: src = h->dmu2[h->cur].p + (size_t)b * h->ld; have = h->ld; break;
    case 6: src = h->dgbuf.p ? h->dgbuf.p + (size_t)b * 84 * 88 : nullptr; have = h->dgbuf.p ? 84L * 88 : 0; break;   // (chained solves: the last chained block of trajectory b, 84 x 88)
    case 5: src = h->dgmu.p; have = h->dgmu.p ? 128L * h->batch : 0; break;   // (chained solves: the means at the positions, all trajectories)
    default: src = h->dmu2[h->cur ^ 1].p + (size_t)b * h->ld; have = h->ld; break;
  }
  if (dst && count > 0 &&
      hipMemcpy(dst, src, sizeof(double) * (size_t)std::min(count, have), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return have;
}

// (diagnostics section of the header; no device needed) the units of the row-slab pass's work queues in
// hand-out order for a batch of `batch` trajectories of `nrb` slabs: what tests/test_cpu_host.py checks for coverage
extern "C" int ekf_debug_pass_units(int batch, int nrb, int nch, int mode, int* out, int cap) {
  if (batch < 1 || nrb < 1 || nch < 1 || mode < 0 || mode > 3 || (cap > 0 && !out)) return -1;
  return debug_pass_units(batch, nrb, nch, mode, out, cap);
}

extern "C" int ekf_last_pass(ekf_handle* h, int* kernel, int* k_tiles, int* streaming) {
  if (!h) return EKF_ERR_ARG;
  if (kernel) *kernel = h->last_kernel;
  if (k_tiles) *k_tiles = h->last_nkt;
  if (streaming) *streaming = h->last_streaming;
  return EKF_OK;
}

// ekf_set_option's names: the handle member each sets and its allowed range (include/ekfslam_hip.h documents them)
struct OptionSpec {
  const char* name;
  int ekf_handle::*member;
  int lo, hi;
};
static const OptionSpec k_options[] = {
    {"flush_every", &ekf_handle::opt_flush_every, 0, 64},
    {"rank_limit", &ekf_handle::opt_rank_limit, 2, KTOT},
    {"pass_kernel", &ekf_handle::opt_pass_kernel, -1, 2},   // (not 1: the producer/consumer form, removed in round 3)
    {"pass_chunk", &ekf_handle::opt_pass_chunk, 0, 4096},
    {"pass_workgroups", &ekf_handle::opt_pass_workgroups, 0, 4096},
    {"pass_rows_per_block", &ekf_handle::opt_rows_per_block, 0, 4096},
    {"pass_streaming", &ekf_handle::opt_streaming, -1, 1},
    {"active_bound", &ekf_handle::opt_active_bound, 0, 1},
    {"small_state", &ekf_handle::opt_small_state, 0, 1},
    {"fused_step", &ekf_handle::opt_fused_step, 0, 2},      // (2, diagnostic: every bounded wait times out; garbage results)
    {"fused_cadence", &ekf_handle::opt_fused_cadence, 0, 1},
    {"col_gather", &ekf_handle::opt_col_gather, 0, 1},
    {"w_from_v", &ekf_handle::opt_w_from_v, 0, 1},
    {"panel_shape", &ekf_handle::opt_panel_shape, 0, 3},
    {"lookahead", &ekf_handle::opt_lookahead, 0, 1},
    {"chain", &ekf_handle::opt_chain, 0, 1},
    {"panel_tform", &ekf_handle::opt_panel_tform, 0, 1},
    {"run_end_flush", &ekf_handle::opt_run_end_flush, 0, 1},
    {"pack_dense", &ekf_handle::opt_pack_dense, 0, 2},
    {"fetch_spin", &ekf_handle::opt_fetch_spin, 0, 1},
    {"fetch_verify", &ekf_handle::opt_fetch_verify, 0, 1},
    {"profile_kernels", &ekf_handle::opt_profile_kernels, 0, 1},
    {"profile_stride", &ekf_handle::profile_stride, 1, 1024},
};

extern "C" int ekf_set_option(ekf_handle* h, const char* name, int value) {
  if (!h || !name) return EKF_ERR_ARG;
  for (const OptionSpec& o : k_options) {
    if (std::strcmp(name, o.name) != 0) continue;
    if (value < o.lo || value > o.hi)
      return fail(h, EKF_ERR_ARG, std::string(o.name) + " must be in [" + std::to_string(o.lo) + ", " + std::to_string(o.hi) + "]");
    if (o.member == &ekf_handle::opt_pass_kernel && value == 1)
      return fail(h, EKF_ERR_ARG, "pass_kernel must be -1 (auto), 0 (column strips) or 2 (row slabs)");
    if (o.member == &ekf_handle::opt_small_state || o.member == &ekf_handle::opt_active_bound) {
      // (the small-state path runs only with nothing pending; the pending ranks were formed under the old active bound)
      HIP_TRY(h, hipSetDevice(h->device));
      if (int rc = flush_pending(h)) return rc;
    }
    h->*o.member = value;
    return EKF_OK;
  }
  return fail(h, EKF_ERR_ARG, std::string("unknown option ") + name);
}

// ---- the hypothesis bank (ekf_hyp_*; k_hyp_solve + k_hyp_rows, k_hyp_fill, k_hyp_compare, k_hyp_adopt: ekf_hypotheses.hip) ----
// One frozen map -- a snapshot of a slot's stored triangle and mean, taken at creation: nothing couples the bank to the handle
// afterwards -- and `count` pose hypotheses on it.  The bank owns its stream; steps are asynchronous on it.  A step is the
// records' upload (one record where motion and observations are shared), k_hyp_solve and k_hyp_rows; what the call launches is
// plan_hyp_step's (ekf_host_plan.h).  ekf_hyp_adopt is the one call that touches a handle again: it waits for the bank's stream,
// applies what is pending on the handle (loc_begin's rule), compares the slot's frozen part with the bank's map on the device and
// only then writes the hypothesis's pose part into the slot, on the handle's stream.  ekf_hypotheses_run steps through records uploaded
// once (ekf_hypotheses_stream_upload), with the resampling gated on the device and, while ekf_hypotheses_log is on, a mixture row per step:
// what it launches is plan_hyp_run's.
struct ekf_hypotheses : ekf::HypBank {
  DeviceConfig dcfg{};            // the source's config, the slot's noise pair folded into rd / qd; no table, no counters
  bool gate = false;              // the bank's NIS gate (dcfg.nis_gate: the threshold)
  hipStream_t stream = nullptr;
  DeviceBuf<double> dmap, dmu;    // the map: one trajectory's stored triangle in the source handle's layout, and its mean
  DeviceBuf<int> dtag;            // the slot's tag-table row (TAGMAX ints; empty where the source had no table)
  DeviceBuf<HypState> dst;
  DeviceBuf<double> dX;           // count x 3 x ldx: the pose rows
  DeviceBuf<LocRec> drec;
  StagedUpload<StepIn> recs;      // a call's records: the pinned copy is rewritten once the previous upload has run
  StagedUpload<double> init;      // ekf_hyp_reset's poses and covariances
  DeviceBuf<unsigned> dcmp;       // ekf_hyp_adopt: the compare's mismatch count
  DeviceBuf<HypWeighOut> dhead;   // ekf_hypotheses_weigh / _resample (made at the first of either): the weights' header,
  DeviceBuf<double> dw;           // the weights,
  DeviceBuf<int> dplan;           // ancestors, offspring and the surplus scan (hyp_resample_ints)
  DeviceBuf<StepIn> dstream;      // ekf_hypotheses_stream_upload: stream_steps x stream_nrec records; _detections_upload: 2 x stream_steps
  AssocConfig acfg{};             // the association's gate and ignore list: the source's at creation (ekf_hypotheses_set_association)
  StagedUpload<DetIn> det;        // ekf_hypotheses_step_detections' window
  DeviceBuf<StepIn> dwin_step;    // ... and what k_hyp_associate leaves of it: the two records,
  DeviceBuf<AssocOut> dwin_assoc; // the matched tags,
  DeviceBuf<LocUnmatched> dwin_un;   // the unmatched ids
  DeviceBuf<unsigned> dwin_flags; // and the window's flag
  bool win_valid = false;         // a single window has run
  DeviceBuf<AssocOut> dstream_assoc;   // a detection stream's per-step AssocOut, LocUnmatched and flag (empty: an index stream)
  DeviceBuf<LocUnmatched> dstream_un;
  DeviceBuf<unsigned> dstream_flags;
  StagedUpload<double> draws;     // ekf_hypotheses_run's z: count x K x 3
  DeviceBuf<HypMixRow> dlog;      // ekf_hypotheses_log: the ring of log_cap rows
  DeviceBuf<HypMixRow> dmix;      // ekf_hypotheses_mixture's scratch row
  StagedUpload<double> uobs;      // an unlabelled step's observations: EKF_MMAX ranges, then EKF_MMAX bearings
  DeviceBuf<StepIn> durec;        // ... the records k_hyp_score leaves, one per hypothesis (made at the first unlabelled step),
  DeviceBuf<int> dassign;         // and the assignment rows, count x EKF_MMAX
  DeviceBuf<double> dquery;       // ekf_hypotheses_associate: the observations, then the destinations that are not pinned
  HypWeighOut host_head{};
  std::vector<HypState> host_st;
  std::string err;
};

static int hyp_fail(ekf_hypotheses* hy, int code, const std::string& msg) {
  if (hy) hy->err = msg; else g_create_error = msg;
  return code;
}
#define HYP_TRY(hy, expr)                                                                  \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return hyp_fail(hy, EKF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define HYP_RES(hy, what, expr)                                                            \
  do {                                                                                     \
    const res::Status s_ = (expr);                                                         \
    if (!s_.ok())                                                                          \
      return hyp_fail(hy, EKF_ERR_HIP, std::string(what) + (s_.bytes ? ": allocation of " + std::to_string(s_.bytes) + " bytes" : std::string()) + \
                                           ": " + hipGetErrorString((hipError_t)s_.err));  \
  } while (0)

static HypView hyp_view(const ekf_hypotheses* hy) {
  return HypView{hy->dmap.p, hy->dmu.p, hy->dst.p, hy->dX.p, hy->drec.p, hy->n, hy->ld, hy->ldx, hy->count};
}

extern "C" const char* ekf_hyp_last_error(ekf_hypotheses* hy) { return hy ? hy->err.c_str() : g_create_error.c_str(); }

static int hyp_free(ekf_hypotheses* hy) {
  (void)hipSetDevice(hy->device);
  if (hy->stream) {
    (void)hipStreamSynchronize(hy->stream);
    (void)hipStreamDestroy(hy->stream);
  }
  delete hy;
  return EKF_OK;
}

extern "C" int ekf_hyp_destroy(ekf_hypotheses* hy) {
  if (!hy) return EKF_ERR_ARG;
  return hyp_free(hy);
}

// the allocations and the snapshot of ekf_hyp_create, on the handle's stream (the source's kernels run there)
static int hyp_build(ekf_handle* h, int b, ekf_hypotheses* hy) {
  HIP_TRY(h, hipStreamCreateWithFlags(&hy->stream, hipStreamNonBlocking));
  const size_t K = (size_t)hy->count;
  RES_TRY(h, "the bank's map", res::ensure_group(nullptr, res::want(hy->dmap, (size_t)hy->pstride), res::want(hy->dmu, (size_t)hy->ld)));
  RES_TRY(h, "the hypotheses", res::ensure_group(nullptr, res::want(hy->dst, K), res::want(hy->dX, K * 3 * (size_t)hy->ldx),
                                                 res::want(hy->drec, K), res::want(hy->dcmp, (size_t)1)));
  HIP_TRY(h, hipMemcpyAsync(hy->dmap.p, h->dP.p + (size_t)b * h->pstride, sizeof(double) * (size_t)hy->pstride, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(hy->dmu.p, h->dmu2[h->cur].p + (size_t)b * h->ld, sizeof(double) * (size_t)hy->ld, hipMemcpyDeviceToDevice, h->stream));
  if (h->dtagmap.p) {
    RES_TRY(h, "the bank's tag-table row", hy->dtag.ensure((size_t)TAGMAX));
    HIP_TRY(h, hipMemcpyAsync(hy->dtag.p, h->dtagmap.p + (size_t)b * TAGMAX, sizeof(int) * TAGMAX, hipMemcpyDeviceToDevice, h->stream));
    hy->has_tags = true;
  }
  launch_hyp_fill(h->stream, hyp_view(hy), nullptr, 0, hy->count, hyp_fill_groups(hy->ldx), hy->bound0);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

extern "C" int ekf_hyp_create(ekf_handle* h, int b, int count, ekf_hypotheses** out) {
  const char* fn = "ekf_hyp_create";
  if (!h) return EKF_ERR_ARG;
  if (!out) return bad_arg(h, fn, "NULL out");
  *out = nullptr;
  if (int rc = check_b(h, b, fn)) return rc;
  if (const char* why = plan_hyp_create(h->n[b], count)) return bad_arg(h, fn, why);
  HIP_TRY(h, hipSetDevice(h->device));
  if (int rc = join_aux(h)) return rc;
  if (int rc = flush_pending(h)) return rc;
  if (int rc = check_internal(h, b, fn)) return rc;
  ekf_hypotheses* hy = new ekf_hypotheses();
  hy->device = h->device;
  hy->n = h->n[b];
  hy->ld = h->ld;
  hy->ldx = h->ld;
  hy->pstride = h->pstride;
  hy->count = count;
  hy->cfg = h->cfg;
  hy->bound0 = h->opt_active_bound ? std::min(h->n[b], std::max(h->neff[b], 3)) : h->n[b];
  hy->bound_hi = hy->bound0;
  hy->dcfg = h->dcfg;
  hy->gate = h->dcfg.gate_rej != nullptr;
  hy->dcfg.gate_rej = nullptr;
  if (h->dcfg.noise) {                                   // the slot's row of the noise table, as the table holds it
    double r[NOISE_ROW];
    noise_row_of(h->noise_ms[(size_t)b], h->noise_qs[(size_t)b], r);
    std::copy_n(r, 3, hy->dcfg.rd);
    std::copy_n(r + 3, 2, hy->dcfg.qd);
  }
  hy->dcfg.noise = nullptr;
  hy->acfg = h->acfg;
  hy->acfg.active_bound = 0;                             // (a hypothesis's bound lives in its HypState: the records' neff is not read)
  if (int rc = hyp_build(h, b, hy)) {
    hyp_free(hy);
    return rc;
  }
  *out = hy;
  return EKF_OK;
}

extern "C" int ekf_hyp_set_nis_gate(ekf_hypotheses* hy, double threshold) {
  if (!hy) return EKF_ERR_ARG;
  if (!(threshold > 0.0)) return hyp_fail(hy, EKF_ERR_ARG, "ekf_hyp_set_nis_gate: the threshold must be > 0 (INFINITY: off)");
  hy->gate = !std::isinf(threshold);
  hy->dcfg.nis_gate = threshold;
  return EKF_OK;
}

static int hyp_step(ekf_hypotheses* hy, const char* fn, bool pred, const double* lin, const double* ang, int motion_stride,
                    const int* idx, const double* range, const double* bearing, const int* m, int stride, int obs_stride) {
  if (!hy) return EKF_ERR_ARG;
  HypStepPlan hp;
  if (const char* why = plan_hyp_step(hy, pred, lin, ang, motion_stride, idx, range, bearing, m, stride, obs_stride, hp))
    return hyp_fail(hy, EKF_ERR_ARG, std::string(fn) + ": " + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  StepIn* hs = nullptr;
  HYP_RES(hy, "the records", hy->recs.begin((size_t)hp.nrec, (size_t)hp.nrec, hy->stream, &hs));
  fill_hyp_records(hy, pred, lin, ang, motion_stride, idx, range, bearing, m, stride, obs_stride, hp, hs);
  HYP_RES(hy, "the records' upload", hy->recs.commit((size_t)hp.nrec, hy->stream));
  hy->bound_hi = hp.bound_hi;
  const HypView v = hyp_view(hy);
  launch_hyp_solve(hy->stream, v, hy->recs.device(), hp.rec_stride, hy->dcfg, hy->gate);
  launch_hyp_rows(hy->stream, v, hp.groups);
  HYP_TRY(hy, hipGetLastError());
  return EKF_OK;
}

extern "C" int ekf_hyp_step(ekf_hypotheses* hy, const double* lin, const double* ang, int motion_stride, const int* idx,
                            const double* range, const double* bearing, const int* m, int stride, int obs_stride) {
  return hyp_step(hy, "ekf_hyp_step", true, lin, ang, motion_stride, idx, range, bearing, m, stride, obs_stride);
}

extern "C" int ekf_hyp_update(ekf_hypotheses* hy, const int* idx, const double* range, const double* bearing, const int* m,
                              int stride, int obs_stride) {
  return hyp_step(hy, "ekf_hyp_update", false, nullptr, nullptr, 0, idx, range, bearing, m, stride, obs_stride);
}

extern "C" int ekf_hyp_reset(ekf_hypotheses* hy, int k0, int count, const double* pose, const double* cov) {
  if (!hy) return EKF_ERR_ARG;
  if (const char* why = plan_hyp_range(hy, k0, count)) return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hyp_reset: ") + why);
  if (count == 0) return EKF_OK;
  std::vector<double> packed(12 * (size_t)count);
  if (const char* why = plan_hyp_reset(hy, k0, count, pose, cov, packed.data()))
    return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hyp_reset: ") + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  double* stage = nullptr;
  HYP_RES(hy, "the reset's poses", hy->init.begin(packed.size(), packed.size(), hy->stream, &stage));
  std::memcpy(stage, packed.data(), sizeof(double) * packed.size());
  HYP_RES(hy, "the reset's upload", hy->init.commit(packed.size(), hy->stream));
  launch_hyp_fill(hy->stream, hyp_view(hy), hy->init.device(), k0, count, hyp_fill_groups(hy->ldx), hy->bound0);
  HYP_TRY(hy, hipGetLastError());
  return EKF_OK;
}

extern "C" int ekf_hyp_sync(ekf_hypotheses* hy) {
  if (!hy) return EKF_ERR_ARG;
  HYP_TRY(hy, hipSetDevice(hy->device));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  return EKF_OK;
}

// Blocking; every output may be NULL.  cov: count x 9, the block mirrored.
extern "C" int ekf_hyp_download(ekf_hypotheses* hy, int k0, int count, double* pose, double* cov, double* loglik, long long* n_obs,
                                long long* n_rej, unsigned* flags) {
  if (!hy) return EKF_ERR_ARG;
  if (const char* why = plan_hyp_range(hy, k0, count)) return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hyp_download: ") + why);
  if (count == 0) return EKF_OK;
  HYP_TRY(hy, hipSetDevice(hy->device));
  hy->host_st.resize((size_t)count);
  HYP_TRY(hy, hipMemcpyAsync(hy->host_st.data(), hy->dst.p + k0, sizeof(HypState) * (size_t)count, hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  for (int i = 0; i < count; ++i) {
    const HypState& s = hy->host_st[(size_t)i];
    if (pose) std::copy_n(s.pose, 3, pose + 3 * (size_t)i);
    if (cov)
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) cov[9 * (size_t)i + 3 * a + c] = s.blk[hyp_blk(std::min(a, c), std::max(a, c))];
    if (loglik) loglik[i] = s.loglik;
    if (n_obs) n_obs[i] = s.n_obs;
    if (n_rej) n_rej[i] = s.n_rej;
    if (flags) flags[i] = s.flags;
  }
  return EKF_OK;
}

extern "C" int ekf_hyp_download_rows(ekf_hypotheses* hy, int k, double* rows, int n) {
  if (!hy) return EKF_ERR_ARG;
  if (const char* why = plan_hyp_range(hy, k, 1)) return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hyp_download_rows: ") + why);
  if (!rows || n != hy->n) return hyp_fail(hy, EKF_ERR_ARG, "ekf_hyp_download_rows: NULL rows, or n is not the map's size");
  HYP_TRY(hy, hipSetDevice(hy->device));
  HYP_TRY(hy, hipMemcpy2DAsync(rows, sizeof(double) * (size_t)n, hy->dX.p + (size_t)k * 3 * hy->ldx, sizeof(double) * (size_t)hy->ldx,
                               sizeof(double) * (size_t)n, 3, hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  HypState s;
  HYP_TRY(hy, hipMemcpy(&s, hy->dst.p + k, sizeof(HypState), hipMemcpyDeviceToHost));
  for (int r = 0; r < 3; ++r)                            // (columns 0..2 of the rows are the pose block, mirrored)
    for (int c = 0; c < 3; ++c) rows[(size_t)r * n + c] = s.blk[hyp_blk(std::min(r, c), std::max(r, c))];
  return EKF_OK;
}

// Hypothesis k's pose, block and rows into slot b of `h`, whose frozen part must be the bank's map bit for bit.  Blocking.
extern "C" int ekf_hyp_adopt(ekf_hypotheses* hy, int k, ekf_handle* h, int b) {
  const char* fn = "ekf_hyp_adopt";
  if (!hy) return EKF_ERR_ARG;
  if (!h) return hyp_fail(hy, EKF_ERR_ARG, "ekf_hyp_adopt: NULL handle");
  if (const char* why = plan_hyp_range(hy, k, 1)) return hyp_fail(hy, EKF_ERR_ARG, std::string(fn) + ": " + why);
  if (int rc = check_b(h, b, fn)) return hyp_fail(hy, rc, h->err);
  if (h->device != hy->device) return hyp_fail(hy, EKF_ERR_ARG, "ekf_hyp_adopt: the handle is on another device");
  if (int rc = check_host_bad(h, fn)) return hyp_fail(hy, rc, h->err);
  HIP_TRY(h, hipSetDevice(h->device));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  if (int rc = join_aux(h)) return hyp_fail(hy, rc, h->err);
  if (int rc = flush_pending(h)) return hyp_fail(hy, rc, h->err);
  if (h->n[b] != hy->n)
    return hyp_fail(hy, EKF_ERR_STATE, "ekf_hyp_adopt: the slot's size " + std::to_string(h->n[b]) + " is not the map's " + std::to_string(hy->n));
  const HypView v = hyp_view(hy);
  double* Pb = h->dP.p + (size_t)b * h->pstride;
  double* mub = h->dmu2[h->cur].p + (size_t)b * h->ld;
  unsigned mismatch = 0;
  HYP_TRY(hy, hipMemsetAsync(hy->dcmp.p, 0, sizeof(unsigned), h->stream));
  launch_hyp_compare(h->stream, v, Pb, mub, h->ld, hyp_compare_groups(hy->n), hy->dcmp.p);
  HYP_TRY(hy, hipGetLastError());
  HYP_TRY(hy, hipMemcpyAsync(&mismatch, hy->dcmp.p, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  HypState s;
  HYP_TRY(hy, hipMemcpyAsync(&s, hy->dst.p + k, sizeof(HypState), hipMemcpyDeviceToHost, h->stream));
  HYP_TRY(hy, hipStreamSynchronize(h->stream));
  if (mismatch)
    return hyp_fail(hy, EKF_ERR_STATE, "ekf_hyp_adopt: the slot's frozen part is not the bank's map: " + std::to_string(mismatch) +
                                           " of its landmark means and stored entries P(a, b), a, b >= 3, differ; nothing was written");
  const int bound = std::min(h->n[b], std::max(h->neff[b], s.bound));
  launch_hyp_adopt(h->stream, v, k, Pb, mub, h->ld, h->dso.p + b, bound, hyp_adopt_groups(hy->n));
  HYP_TRY(hy, hipGetLastError());
  h->neff[b] = bound;
  h->neff_enq[b] = h->opt_active_bound ? h->neff[b] : h->n[b];
  HYP_TRY(hy, hipStreamSynchronize(h->stream));
  return EKF_OK;
}

// ---- weights and resampling (k_hyp_weigh, k_hyp_plan, k_hyp_copy, k_hyp_split; shapes: plan_hyp_resample) ----
// The scratch of both calls, made at the first: a header, count weights, 3 count ints.
static int hyp_resample_view(ekf_hypotheses* hy, HypResampleView& rs) {
  const size_t K = (size_t)hy->count;
  HYP_RES(hy, "the resampling's scratch", res::ensure_group(nullptr, res::want(hy->dhead, (size_t)1), res::want(hy->dw, K),
                                                            res::want(hy->dplan, hyp_resample_ints(hy->count))));
  rs = HypResampleView{hy->dhead.p, hy->dw.p, hy->dplan.p, hy->dplan.p + K, hy->dplan.p + 2 * K};
  return EKF_OK;
}

// k_hyp_copy's stores: nontemporal unless EKFSLAM_HIP_HYP_COPY_NT=0 (tools/hyp_resample_time.py measures both,
// profiles/hyp_resample.txt)
static bool hyp_copy_nt() {
  const char* e = std::getenv("EKFSLAM_HIP_HYP_COPY_NT");
  return e ? std::atoi(e) != 0 : true;
}

// the header into ess / logmean / live, the plan into ancestors / offspring: blocks if any of them is asked for
static int hyp_resample_outputs(ekf_hypotheses* hy, const HypResampleView& rs, int* ancestors, int* offspring, double* ess,
                                double* logmean, int* live) {
  if (!ancestors && !offspring && !ess && !logmean && !live) return EKF_OK;
  const size_t K = (size_t)hy->count;
  if (ess || logmean || live)
    HYP_TRY(hy, hipMemcpyAsync(&hy->host_head, rs.head, sizeof(HypWeighOut), hipMemcpyDeviceToHost, hy->stream));
  if (ancestors) HYP_TRY(hy, hipMemcpyAsync(ancestors, rs.anc, sizeof(int) * K, hipMemcpyDeviceToHost, hy->stream));
  if (offspring) HYP_TRY(hy, hipMemcpyAsync(offspring, rs.off, sizeof(int) * K, hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  if (ess) *ess = hy->host_head.ess;
  if (logmean) *logmean = hy->host_head.logmean;
  if (live) *live = hy->host_head.live;
  return EKF_OK;
}

extern "C" int ekf_hypotheses_weigh(ekf_hypotheses* hy, double* ess, double* logmean, int* live) {
  if (!hy) return EKF_ERR_ARG;
  HYP_TRY(hy, hipSetDevice(hy->device));
  HypResampleView rs;
  if (int rc = hyp_resample_view(hy, rs)) return rc;
  launch_hyp_weigh(hy->stream, hyp_view(hy), rs, hyp_plan_chunk(hy->count));
  HYP_TRY(hy, hipGetLastError());
  return hyp_resample_outputs(hy, rs, nullptr, nullptr, ess, logmean, live);
}

extern "C" int ekf_hypotheses_resample(ekf_hypotheses* hy, double u, double split, const double* z, int* ancestors, int* offspring,
                                       double* ess, double* logmean) {
  if (!hy) return EKF_ERR_ARG;
  HypResamplePlan rp;
  if (const char* why = plan_hyp_resample(hy, u, split, z, rp))
    return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hypotheses_resample: ") + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  HypResampleView rs;
  if (int rc = hyp_resample_view(hy, rs)) return rc;
  if (rp.split) {                                        // (before the first launch: a failed upload leaves the bank alone)
    const size_t nz = 3 * (size_t)hy->count;
    double* stage = nullptr;
    HYP_RES(hy, "the split's draws", hy->init.begin(nz, 12 * (size_t)hy->count, hy->stream, &stage));
    std::memcpy(stage, z, sizeof(double) * nz);
    HYP_RES(hy, "the draws' upload", hy->init.commit(nz, hy->stream));
  }
  const HypView v = hyp_view(hy);
  launch_hyp_weigh(hy->stream, v, rs, rp.chunk);
  launch_hyp_plan(hy->stream, v, rs, rp);
  launch_hyp_copy(hy->stream, hyp_copy_nt(), v, rs, rp);
  if (rp.split) launch_hyp_split(hy->stream, v, rs, rp, hy->init.device());
  HYP_TRY(hy, hipGetLastError());
  return hyp_resample_outputs(hy, rs, ancestors, offspring, ess, logmean, nullptr);
}

// ---- the uploaded stream, its run, the mixture and its log (plan_hyp_stream, plan_hyp_run, plan_hyp_log; k_hyp_mixture) ----
// An allocation of `what` failed: the message with the byte count; the runtime's sticky error is cleared, the bank stays usable.
static int hyp_alloc_fail(ekf_hypotheses* hy, const std::string& what, const res::Status& s) {
  (void)hipGetLastError();
  return hyp_fail(hy, EKF_ERR_HIP, what + ": allocation of " + std::to_string(s.bytes) + " bytes: " + hipGetErrorString((hipError_t)s.err));
}

// The uploaded stream of either kind released (a run in flight still reads the old records: release_group waits for the
// stream) and the bank's mirror of it cleared: the bank stays usable without a stream.
static int hyp_stream_drop(ekf_hypotheses* hy, const char* fn) {
  HYP_RES(hy, fn, res::release_group<HipBackend>(hy->stream, hy->dstream, hy->dstream_assoc, hy->dstream_un, hy->dstream_flags));
  hy->stream_steps = 0;
  hy->stream_bound.clear();
  hy->stream_passes.clear();
  hy->stream_pass_stride = 0;
  return EKF_OK;
}

// Blocking.  The map is frozen, so nothing the bank does afterwards makes the records stale.
extern "C" int ekf_hypotheses_stream_upload(ekf_hypotheses* hy, int steps, const double* lin, const double* ang, int motion_stride,
                                     const int* idx, const double* range, const double* bearing, const int* m, int stride,
                                     int obs_stride) {
  if (!hy) return EKF_ERR_ARG;
  HypStreamPlan sp;
  if (const char* why = plan_hyp_stream(hy, steps, lin, ang, motion_stride, idx, range, bearing, m, stride, obs_stride, sp))
    return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hypotheses_stream_upload: ") + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  std::vector<StepIn> recs(sp.records());
  fill_hyp_stream(hy, lin, ang, motion_stride, idx, range, bearing, m, stride, obs_stride, sp, recs.data());
  if (int rc = hyp_stream_drop(hy, "ekf_hypotheses_stream_upload")) return rc;
  if (sp.steps == 0) return EKF_OK;
  if (const res::Status s = hy->dstream.ensure(sp.records()); !s.ok())
    return hyp_alloc_fail(hy, "ekf_hypotheses_stream_upload: the stream of " + std::to_string(sp.steps) + " steps", s);
  HYP_TRY(hy, hipMemcpyAsync(hy->dstream.p, recs.data(), sizeof(StepIn) * recs.size(), hipMemcpyHostToDevice, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  hy->stream_steps = sp.steps;
  hy->stream_nrec = sp.nrec;
  hy->stream_rec_stride = sp.rec_stride;
  hy->stream_bound = std::move(sp.bound);
  return EKF_OK;
}

// Asynchronous on the bank's stream: plain stream-ordered launches, each behind the one before it.  Blocks only in the draws'
// StagedUpload, where the previous call's upload has not run yet.
extern "C" int ekf_hypotheses_run(ekf_hypotheses* hy, int first, int count, double ess_fraction, double split, const double* u,
                           const double* z) {
  if (!hy) return EKF_ERR_ARG;
  if (!hyp_stream_loaded(hy)) return hyp_fail(hy, EKF_ERR_STATE, "ekf_hypotheses_run: no stream uploaded (ekf_hypotheses_stream_upload / ekf_hypotheses_detections_upload)");
  HypRunPlan rp;
  if (const char* why = plan_hyp_run(hy, first, count, ess_fraction, split, u, z, rp))
    return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hypotheses_run: ") + why);
  if (count == 0) return EKF_OK;
  HYP_TRY(hy, hipSetDevice(hy->device));
  HypResampleView rs{};
  if (rp.weigh)
    if (int rc = hyp_resample_view(hy, rs)) return rc;
  const size_t nz = 3 * (size_t)hy->count;               // a step's draws
  if (rp.rs.split) {                                     // (before the first launch: a failed upload leaves the bank alone)
    double* stage = nullptr;
    HYP_RES(hy, "the run's draws", hy->draws.begin(nz * (size_t)count, nz * (size_t)count, hy->stream, &stage));
    std::memcpy(stage, z, sizeof(double) * nz * (size_t)count);
    HYP_RES(hy, "the draws' upload", hy->draws.commit(nz * (size_t)count, hy->stream));
  }
  const HypView v = hyp_view(hy);
  const bool nt = hyp_copy_nt();
  HypResamplePlan step = rp.rs;
  for (int i = 0; i < count; ++i) {
    for (int p = 0; p < rp.passes[(size_t)i]; ++p) {     // (a detection stream's step with more than MMAX tags: two)
      launch_hyp_solve(hy->stream, v, hy->dstream.p + rp.rec_offset(i, p), rp.rec_stride, hy->dcfg, hy->gate);
      launch_hyp_rows(hy->stream, v, rp.groups[(size_t)i]);
    }
    if (rp.weigh) launch_hyp_weigh(hy->stream, v, rs, step.chunk);
    if (rp.mixture) launch_hyp_mixture(hy->stream, v, rs, step, hy->dlog.p + (hy->log_steps + i) % hy->log_cap);
    if (rp.resample) {
      step.u = u[i];
      launch_hyp_plan(hy->stream, v, rs, step);
      launch_hyp_copy(hy->stream, nt, v, rs, step);
      if (step.split) launch_hyp_split(hy->stream, v, rs, step, hy->draws.device() + nz * (size_t)i);
    }
  }
  hy->bound_hi = rp.bound_hi;
  if (rp.mixture) hy->log_steps += count;
  HYP_TRY(hy, hipGetLastError());
  return EKF_OK;
}

// a row into the outputs' entry i (each may be NULL); the covariance mirrored to 3 x 3
static void hyp_row_out(const HypMixRow& r, size_t i, double* mean, double* cov, double* ess, double* logmean, int* live, int* best,
                        int* resampled) {
  if (mean) std::copy_n(r.mean, 3, mean + 3 * i);
  if (cov)
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) cov[9 * i + 3 * a + c] = r.cov[hyp_blk(std::min(a, c), std::max(a, c))];
  if (ess) ess[i] = r.ess;
  if (logmean) logmean[i] = r.logmean;
  if (live) live[i] = r.live;
  if (best) best[i] = r.best;
  if (resampled) resampled[i] = r.resampled;
}

// Blocking.  k_hyp_weigh + k_hyp_mixture on the bank as it stands, into scratch every later call forms anew.
extern "C" int ekf_hypotheses_mixture(ekf_hypotheses* hy, double* mean, double* cov, double* ess, double* logmean, int* live, int* best) {
  if (!hy) return EKF_ERR_ARG;
  HYP_TRY(hy, hipSetDevice(hy->device));
  HypResampleView rs;
  if (int rc = hyp_resample_view(hy, rs)) return rc;
  if (const res::Status s = hy->dmix.ensure(1); !s.ok()) return hyp_alloc_fail(hy, "ekf_hypotheses_mixture: the row", s);
  HypResamplePlan rp;
  rp.chunk = hyp_plan_chunk(hy->count);
  rp.ess_min = 0.0;                                      // (no resampling stands behind this row)
  const HypView v = hyp_view(hy);
  launch_hyp_weigh(hy->stream, v, rs, rp.chunk);
  launch_hyp_mixture(hy->stream, v, rs, rp, hy->dmix.p);
  HYP_TRY(hy, hipGetLastError());
  HypMixRow r;
  HYP_TRY(hy, hipMemcpyAsync(&r, hy->dmix.p, sizeof(HypMixRow), hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  hyp_row_out(r, 0, mean, cov, ess, logmean, live, best, nullptr);
  return EKF_OK;
}

// ekf_log_poses' design for the bank: a device ring of the last `capacity` rows, written by ekf_hypotheses_run's steps only.
extern "C" int ekf_hypotheses_log(ekf_hypotheses* hy, int capacity) {
  if (!hy) return EKF_ERR_ARG;
  if (const char* why = plan_hyp_log(capacity)) return hyp_fail(hy, EKF_ERR_ARG, std::string("ekf_hypotheses_log: ") + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  // (launches in flight still write the old ring: release_group waits for the stream)
  HYP_RES(hy, "ekf_hypotheses_log", res::release_group<HipBackend>(hy->stream, hy->dlog));
  hy->log_cap = 0;
  hy->log_steps = 0;
  if (capacity == 0) return EKF_OK;
  if (const res::Status s = hy->dlog.ensure((size_t)capacity); !s.ok())
    return hyp_alloc_fail(hy, "ekf_hypotheses_log: the ring of " + std::to_string(capacity) + " steps", s);
  hy->log_cap = capacity;
  return EKF_OK;
}

extern "C" int ekf_hypotheses_log_steps(ekf_hypotheses* hy, long long* logged) {
  if (!hy || !logged) return EKF_ERR_ARG;
  *logged = hy->log_steps;
  return EKF_OK;
}

// Blocking and stream-ordered; every output may be NULL.
extern "C" int ekf_hypotheses_download_log(ekf_hypotheses* hy, long long first, int count, double* mean, double* cov, double* ess,
                                    double* logmean, int* live, int* best, int* resampled) {
  if (!hy) return EKF_ERR_ARG;
  if (!hy->dlog.p) return hyp_fail(hy, EKF_ERR_STATE, "ekf_hypotheses_download_log: the log is off (ekf_hypotheses_log)");
  if (!ring_range_ok(first, count, hy->log_steps, hy->log_cap))
    return hyp_fail(hy, EKF_ERR_ARG, "ekf_hypotheses_download_log: steps [" + std::to_string(first) + ", " + std::to_string(first + count) +
                                         ") are not among the last " + std::to_string(hy->log_cap) + " of the " +
                                         std::to_string(hy->log_steps) + " logged");
  if (count == 0) return EKF_OK;
  HYP_TRY(hy, hipSetDevice(hy->device));
  std::vector<HypMixRow> hr((size_t)count);
  const RingPieces rp = ring_pieces(first, count, hy->log_cap);
  for (int i = 0; i < rp.n; ++i) {
    const RingPieces::Piece& c = rp.piece[i];
    HYP_TRY(hy, hipMemcpyAsync(hr.data() + c.done, hy->dlog.p + c.slot, sizeof(HypMixRow) * (size_t)c.rows, hipMemcpyDeviceToHost, hy->stream));
  }
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  for (size_t i = 0; i < hr.size(); ++i) hyp_row_out(hr[i], i, mean, cov, ess, logmean, live, best, resampled);
  return EKF_OK;
}

// ---- a bank's windows of raw detections (plan_hyp_detections, plan_hyp_detection_stream; k_hyp_associate: ekf_loc_assoc.hip) ----
// The bank's tag-table row and its map are frozen and the walk of a window reads no pose, so a window is associated ONCE for
// every hypothesis: k_hyp_associate leaves the shared records k_hyp_solve reads with rec_stride 0.  A single window is staged and
// associated in front of its solves, asynchronously; a whole stream is associated at its upload, in one launch, and
// ekf_hypotheses_run then runs it as it runs an index stream.  A later ekf_hypotheses_set_association reaches later calls and
// uploads only: an uploaded stream is not associated again.
extern "C" int ekf_hypotheses_set_association(ekf_hypotheses* hy, double gate_range, const int* ignore_tags, int n_ignore) {
  if (!hy) return EKF_ERR_ARG;
  if (n_ignore < 0 || n_ignore > IGNMAX || (n_ignore > 0 && !ignore_tags))
    return hyp_fail(hy, EKF_ERR_ARG, "ekf_hypotheses_set_association: at most 16 ignored tags");
  hy->acfg.gate2 = gate_range * gate_range;
  hy->acfg.n_ignore = n_ignore;
  for (int i = 0; i < n_ignore; ++i) hy->acfg.ignore[i] = ignore_tags[i];
  return EKF_OK;
}

// Asynchronous on the bank's stream: the window's upload, k_hyp_associate on it, then the planned solve / rows pairs on the two
// shared records.  A second pass whose record turns out empty (fewer than MMAX + 1 tags matched) applies nothing: k_hyp_solve
// leaves the HypState and k_hyp_rows leaves at once (LocRec::apply).
extern "C" int ekf_hypotheses_step_detections(ekf_hypotheses* hy, double lin, double ang, int count, const int* tag_id,
                                              const double* pose_t, const double* pose_err) {
  const char* fn = "ekf_hypotheses_step_detections";
  if (!hy) return EKF_ERR_ARG;
  HypDetPlan dp;
  if (const char* why = plan_hyp_detections(hy, lin, ang, count, tag_id, pose_t, pose_err, dp))
    return hyp_fail(hy, dp.code, std::string(fn) + ": " + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  bool fresh = false;
  HYP_RES(hy, "the window's records", res::ensure_group(&fresh, res::want(hy->dwin_step, (size_t)2), res::want(hy->dwin_assoc, (size_t)1),
                                                        res::want(hy->dwin_un, (size_t)1), res::want(hy->dwin_flags, (size_t)1)));
  if (fresh) HYP_TRY(hy, hipMemsetAsync(hy->dwin_assoc.p, 0, sizeof(AssocOut), hy->stream));   // (the kernel writes the m slots taken)
  DetIn* hs = nullptr;
  HYP_RES(hy, "the window", hy->det.begin(1, 1, hy->stream, &hs));
  fill_hyp_det_records(1, &lin, &ang, &count, tag_id, pose_t, pose_err, count, hs);
  HYP_RES(hy, "the window's upload", hy->det.commit(1, hy->stream));
  const HypView v = hyp_view(hy);
  launch_hyp_associate(hy->stream, v, hy->dtag.p, hy->det.device(), 1, hy->dwin_step.p, hy->dwin_assoc.p, hy->dwin_un.p,
                       hy->dwin_flags.p, hy->acfg);
  hy->win_valid = true;
  hy->bound_hi = dp.bound_hi;
  for (int p = 0; p < dp.passes; ++p) {
    launch_hyp_solve(hy->stream, v, hy->dwin_step.p + p, 0, hy->dcfg, hy->gate);
    launch_hyp_rows(hy->stream, v, dp.groups);
  }
  HYP_TRY(hy, hipGetLastError());
  return EKF_OK;
}

// Blocking.  The windows are copied and associated in one launch (a wave per window); the records stay as the bank's stream with
// each step's AssocOut, LocUnmatched and flag, and each step's matched count and highest landmark come back, so that a run's
// bounds and passes are exact.  Replaces an earlier stream of either kind; a refused call leaves it.
extern "C" int ekf_hypotheses_detections_upload(ekf_hypotheses* hy, int steps, const double* lin, const double* ang, const int* count,
                                                const int* tag_id, const double* pose_t, const double* pose_err, int stride) {
  const char* fn = "ekf_hypotheses_detections_upload";
  if (!hy) return EKF_ERR_ARG;
  HypDetStreamPlan sp;
  if (const char* why = plan_hyp_detection_stream(hy, steps, lin, ang, count, tag_id, pose_t, pose_err, stride, sp))
    return hyp_fail(hy, sp.code, std::string(fn) + ": " + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  std::vector<DetIn> wins((size_t)sp.steps);
  fill_hyp_det_records(sp.steps, lin, ang, count, tag_id, pose_t, pose_err, stride, wins.data());
  if (int rc = hyp_stream_drop(hy, fn)) return rc;
  if (sp.steps == 0) return EKF_OK;
  const size_t S = (size_t)sp.steps;
  DeviceBuf<DetIn> ddet;                                 // (the windows themselves are not kept)
  if (const res::Status s = res::ensure_group(nullptr, res::want(hy->dstream, sp.records()), res::want(hy->dstream_assoc, S),
                                              res::want(hy->dstream_un, S), res::want(hy->dstream_flags, S), res::want(ddet, S));
      !s.ok())
    return hyp_alloc_fail(hy, std::string(fn) + ": the stream of " + std::to_string(sp.steps) + " windows", s);
  hipError_t e = hipMemsetAsync(hy->dstream_assoc.p, 0, sizeof(AssocOut) * S, hy->stream);   // (the kernel writes the slots taken)
  if (e == hipSuccess) e = hipMemcpyAsync(ddet.p, wins.data(), sizeof(DetIn) * S, hipMemcpyHostToDevice, hy->stream);
  std::vector<AssocOut> ao(S);
  if (e == hipSuccess) {
    launch_hyp_associate(hy->stream, hyp_view(hy), hy->dtag.p, ddet.p, sp.steps, hy->dstream.p, hy->dstream_assoc.p,
                         hy->dstream_un.p, hy->dstream_flags.p, hy->acfg);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(ao.data(), hy->dstream_assoc.p, sizeof(AssocOut) * S, hipMemcpyDeviceToHost, hy->stream);
  const hipError_t es = hipStreamSynchronize(hy->stream);   // (also on a failure: ddet and the host arrays leave with this call)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    (void)hyp_stream_drop(hy, fn);
    return hyp_fail(hy, EKF_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  }
  finish_hyp_detection_stream(hy, ao.data(), sp);
  hy->stream_steps = sp.steps;
  hy->stream_nrec = 1;
  hy->stream_rec_stride = 0;
  hy->stream_bound = std::move(sp.bound);
  hy->stream_passes = std::move(sp.passes);
  hy->stream_pass_stride = S;
  return EKF_OK;
}

// Blocking; every output may be NULL.  idx / tag_id / err / range / bearing and unmatched: EKF_AMAX entries each.
extern "C" int ekf_hypotheses_download_tags(ekf_hypotheses* hy, int step, int* m, int* idx, int* tag_id, double* err, double* range,
                                            double* bearing, int* n_unmatched, int* unmatched, unsigned* flags) {
  if (!hy) return EKF_ERR_ARG;
  int code = EKF_ERR_ARG;
  if (const char* why = plan_hyp_download_tags(hy, step, hy->win_valid, &code))
    return hyp_fail(hy, code, std::string("ekf_hypotheses_download_tags: ") + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  const bool single = step < 0;
  const size_t at = single ? 0 : (size_t)step;
  AssocOut a;
  LocUnmatched u;
  unsigned f = 0;
  HYP_TRY(hy, hipMemcpyAsync(&a, (single ? hy->dwin_assoc.p : hy->dstream_assoc.p) + at, sizeof(a), hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipMemcpyAsync(&u, (single ? hy->dwin_un.p : hy->dstream_un.p) + at, sizeof(u), hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipMemcpyAsync(&f, (single ? hy->dwin_flags.p : hy->dstream_flags.p) + at, sizeof(f), hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  if (m) *m = a.m;
  for (int i = 0; i < AMAX; ++i) {
    if (idx) idx[i] = a.idx[i];
    if (tag_id) tag_id[i] = a.tag_id[i];
    if (err) err[i] = a.err[i];
    if (range) range[i] = a.range[i];
    if (bearing) bearing[i] = a.bearing[i];
    if (unmatched) unmatched[i] = u.tag_id[i];
  }
  if (n_unmatched) *n_unmatched = u.total;
  if (flags) *flags = f;
  return EKF_OK;
}

// ---- a bank's unlabelled observations (plan_hyp_associate, plan_hyp_unlabelled; k_hyp_score: ekf_hyp_assoc.hip) ----
// The query is a read-only query of the bank as ekf_associate is one of a handle -- the Query scaffold with the bank's own
// staging buffer, on the bank's stream --; a step from unlabelled observations is ekf_hyp_step's prediction, k_hyp_score writing
// one record and one assignment row per hypothesis on the device, then the bank's solve and row launches on those records: no
// host round trip.  The records, the assignment rows and the staging buffer are made at the first call that needs them.
static int hyp_unlabelled_scratch(ekf_hypotheses* hy, const char* fn) {
  const size_t K = (size_t)hy->count;
  HYP_RES(hy, std::string(fn) + ": the records and assignment rows",
          res::ensure_group(nullptr, res::want(hy->durec, K), res::want(hy->dassign, K * (size_t)MMAX)));
  return EKF_OK;
}

// Blocking, stream-ordered behind the bank's stream; changes nothing a later call can see.
extern "C" int ekf_hypotheses_associate(ekf_hypotheses* hy, int k0, int count, const double* range, const double* bearing, int m,
                                        int* cand, double* cand_nis, double* cand_logdet, double* min_nis, double* all_nis,
                                        double* all_logdet, int cap) {
  const char* fn = "ekf_hypotheses_associate";
  if (!hy) return EKF_ERR_ARG;
  HypAssocPlan ap;
  if (const char* why = plan_hyp_associate(hy, k0, count, range, bearing, m, cand, all_nis, all_logdet, cap, ap))
    return hyp_fail(hy, EKF_ERR_ARG, std::string(fn) + ": " + why);
  if (count == 0 || m == 0) return EKF_OK;               // (every output is empty)
  HYP_TRY(hy, hipSetDevice(hy->device));
  const size_t obs = (size_t)count * (size_t)m, full_words = obs * (size_t)ap.cap_eff;
  Query q{};
  q.plan.inputs = 2 * (size_t)MMAX;                      // range, bearing
  q.add(cand, obs);                                      // (2 ints per observation)
  q.add(cand_nis, obs * 2);
  q.add(cand_logdet, obs * 2);
  q.add(min_nis, obs);
  q.add(all_nis, full_words);
  q.add(all_logdet, full_words);
  HYP_RES(hy, std::string(fn) + ": the staging buffer", hy->dquery.reserve(plan_staging(q.plan), 0, hy->stream));
  for (int i = 0; i < q.plan.ndst; ++i)
    if (q.plan.dst[i].staged) q.dev[i] = hy->dquery.p + q.plan.dst[i].at;
  double *dzr = hy->dquery.p, *dzb = dzr + MMAX;
  HYP_TRY(hy, hipMemcpyAsync(dzr, range, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, hy->stream));
  HYP_TRY(hy, hipMemcpyAsync(dzb, bearing, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, hy->stream));
  const HypScoreOut o{q.out<int>(0), q.out<double>(1), q.out<double>(2), q.out<double>(3), q.out<double>(4), q.out<double>(5),
                      ap.cap_eff, nullptr, nullptr, 0.0, 0.0};
  launch_hyp_score(hy->stream, hyp_view(hy), hy->dcfg, k0, count, ap.chunks, dzr, dzb, m, o);
  HYP_TRY(hy, hipGetLastError());
  for (int i = 0; i < q.plan.ndst; ++i)
    if (q.plan.dst[i].staged)
      HYP_TRY(hy, hipMemcpyAsync(q.host[i], q.dev[i], sizeof(double) * q.plan.dst[i].words, hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  return EKF_OK;
}

static int hyp_unlabelled(ekf_hypotheses* hy, const char* fn, bool pred, const double* lin, const double* ang, int motion_stride,
                          const double* range, const double* bearing, int m, double accept, double miss) {
  if (!hy) return EKF_ERR_ARG;
  HypUnlabelledPlan up;
  if (const char* why = plan_hyp_unlabelled(hy, pred, lin, ang, motion_stride, range, bearing, m, accept, miss, up))
    return hyp_fail(hy, EKF_ERR_ARG, std::string(fn) + ": " + why);
  HYP_TRY(hy, hipSetDevice(hy->device));
  if (int rc = hyp_unlabelled_scratch(hy, fn)) return rc;
  double* zs = nullptr;
  HYP_RES(hy, std::string(fn) + ": the observations", hy->uobs.begin(2 * (size_t)MMAX, 2 * (size_t)MMAX, hy->stream, &zs));
  if (pred) {                                            // ekf_hyp_step's two launches on a prediction-only record
    const int none = 0;
    if (int rc = hyp_step(hy, fn, true, lin, ang, motion_stride, nullptr, nullptr, nullptr, &none, 0, 0)) return rc;
  }
  for (int q = 0; q < MMAX; ++q) {
    zs[q] = q < up.m ? range[q] : 0.0;
    zs[MMAX + q] = q < up.m ? bearing[q] : 0.0;
  }
  HYP_RES(hy, std::string(fn) + ": the observations' upload", hy->uobs.commit(2 * (size_t)MMAX, hy->stream));
  const HypView v = hyp_view(hy);
  const HypScoreOut o{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, hy->durec.p, hy->dassign.p, accept, miss};
  launch_hyp_score(hy->stream, v, hy->dcfg, 0, hy->count, up.chunks, hy->uobs.device(), hy->uobs.device() + MMAX, up.m, o);
  hy->unlabelled_run = true;
  hy->bound_hi = up.bound_hi;
  launch_hyp_solve(hy->stream, v, hy->durec.p, 1, hy->dcfg, hy->gate);
  launch_hyp_rows(hy->stream, v, up.groups);
  HYP_TRY(hy, hipGetLastError());
  return EKF_OK;
}

// Asynchronous on the bank's stream.
extern "C" int ekf_hypotheses_step_unlabelled(ekf_hypotheses* hy, const double* lin, const double* ang, int motion_stride,
                                              const double* range, const double* bearing, int m, double accept, double miss) {
  return hyp_unlabelled(hy, "ekf_hypotheses_step_unlabelled", true, lin, ang, motion_stride, range, bearing, m, accept, miss);
}

extern "C" int ekf_hypotheses_update_unlabelled(ekf_hypotheses* hy, const double* range, const double* bearing, int m, double accept,
                                                double miss) {
  return hyp_unlabelled(hy, "ekf_hypotheses_update_unlabelled", false, nullptr, nullptr, 0, range, bearing, m, accept, miss);
}

// Blocking.  assign: count x EKF_MMAX, the landmark of every accepted observation of the last unlabelled step, -1 elsewhere.
extern "C" int ekf_hypotheses_download_assignment(ekf_hypotheses* hy, int k0, int count, int* assign) {
  if (!hy) return EKF_ERR_ARG;
  int code = EKF_ERR_ARG;
  if (const char* why = plan_hyp_assignment(hy, k0, count, assign, &code))
    return hyp_fail(hy, code, std::string("ekf_hypotheses_download_assignment: ") + why);
  if (count == 0) return EKF_OK;
  HYP_TRY(hy, hipSetDevice(hy->device));
  HYP_TRY(hy, hipMemcpyAsync(assign, hy->dassign.p + (size_t)k0 * MMAX, sizeof(int) * (size_t)count * MMAX, hipMemcpyDeviceToHost, hy->stream));
  HYP_TRY(hy, hipStreamSynchronize(hy->stream));
  return EKF_OK;
}

// (diagnostics section of the header) the query's launch alone, `reps` times between one event pair on the bank's stream
extern "C" int ekf_debug_hyp_score_time(ekf_hypotheses* hy, const double* range, const double* bearing, int m, int reps,
                                        double* us_per_launch) {
  const char* fn = "ekf_debug_hyp_score_time";
  if (!hy) return EKF_ERR_ARG;
  int cand_probe = 0;
  HypAssocPlan ap;
  if (const char* why = plan_hyp_associate(hy, 0, hy->count, range, bearing, m, &cand_probe, nullptr, nullptr, 0, ap))
    return hyp_fail(hy, EKF_ERR_ARG, std::string(fn) + ": " + why);
  if (reps < 1 || !us_per_launch) return hyp_fail(hy, EKF_ERR_ARG, std::string(fn) + ": reps must be >= 1 and us_per_launch given");
  HYP_TRY(hy, hipSetDevice(hy->device));
  const size_t obs = (size_t)hy->count * (size_t)std::max(m, 1);
  HYP_RES(hy, std::string(fn) + ": the staging buffer", hy->dquery.reserve(2 * (size_t)MMAX + 6 * obs, 0, hy->stream));
  double *dzr = hy->dquery.p, *dzb = dzr + MMAX, *out = dzb + MMAX;
  if (m > 0) {
    HYP_TRY(hy, hipMemcpyAsync(dzr, range, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, hy->stream));
    HYP_TRY(hy, hipMemcpyAsync(dzb, bearing, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, hy->stream));
  }
  const HypScoreOut o{reinterpret_cast<int*>(out), out + obs, out + 3 * obs, out + 5 * obs, nullptr, nullptr, 0, nullptr, nullptr, 0.0, 0.0};
  res::Event<HipBackend> t0, t1;
  HYP_RES(hy, "t0", t0.ensure(true));
  HYP_RES(hy, "t1", t1.ensure(true));
  HYP_RES(hy, "t0", t0.record(hy->stream));
  for (int r = 0; r < reps; ++r) launch_hyp_score(hy->stream, hyp_view(hy), hy->dcfg, 0, hy->count, ap.chunks, dzr, dzb, m, o);
  HYP_RES(hy, "t1", t1.record(hy->stream));
  HYP_TRY(hy, hipGetLastError());
  HYP_RES(hy, "t1", t1.wait_if_recorded());
  float ms = 0.f;
  HYP_TRY(hy, hipEventElapsedTime(&ms, t0.ev, t1.ev));
  *us_per_launch = 1e3 * (double)ms / reps;
  return EKF_OK;
}
