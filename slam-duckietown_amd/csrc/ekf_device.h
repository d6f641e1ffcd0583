// Shared host/device records of the EKF-SLAM core (gfx950 only).
#pragma once
#ifdef EKF_HOST_ONLY                                     /* plain g++ (the sanitizer build of the host logic, tests/host_plan_check.cpp) */
#define __host__
#define __device__
#define __forceinline__ inline
#else
#include <hip/hip_runtime.h>
#endif
#include <cstddef>
#include "../../include/ekfslam_hip.h"

namespace ekf {

constexpr int MMAX = EKF_MMAX;          // landmarks per update pass
constexpr int CMAX = 3 + 2 * MMAX;      // compressed sub-state size (35)
constexpr int KTOT = 80;                // rank slots of the deferred low-rank update  P = P_base + W V
constexpr int NKT = KTOT / 4;           // the same in MFMA k-tiles (v_mfma_f64_16x16x4)

// ranks one step appends: 2 per observed landmark (the prediction only changes rows 0,1 of the stored
// triangle and is applied to P_base directly); steps are packed back to back and only the total is padded
// to a whole k-tile (the step that is last so far zero-fills the pad ranks)
__host__ __device__ constexpr int ranks_for(int mcap) { return 2 * mcap; }

// ---- size limits of the small-state path (ekf_small.hip: the kernel's LDS, ekf_host_plan.h: small_state_limit) ----
constexpr int SMALL_N_MAX = 79;         // 3 + 2 * 38 (<= 5 column tiles of 16; 50 KB of LDS): beyond, the general kernels are faster
                                        // for ONE trajectory (latency) ...
constexpr int SMALL_N_MAX_BANK = 131;   // ... but not for a bank that fills the chip (3 + 2 * 64; 9 column tiles, 137 KB of LDS: one
constexpr int SMALL_BANK_MIN = 128;     // workgroup per CU): N = 64 x 256 10.4 M against 7.9 M steps/s, x 1024 against 5.4 M

// ---- layout of one trajectory's P_base (round 4) ----
// Row-major with row stride ld while ld <= 4096 (ld is then a power of two).  Beyond that the covariance is cut into
// COLUMN PANELS of PPW = 4096 doubles: panel p holds the columns [4096 p, 4096 (p + 1)) of every row, row-major with a row
// stride of exactly 4096 doubles (32 KB), panels ld x 4096 doubles apart (rows == ld there):
//     index(i, j) = (j >> 12) * (ld * 4096) + i * min(ld, 4096) + (j & 4095)
// -- one formula for both cases (j < ld <= 4096 leaves the panel term at zero).  Why: the sixteen 512-byte row segments of
// a 16 x 64 tile of the covariance pass then lie 32 KB apart whatever the size of the state, the pitch the pass streams
// best at (N = 2000, ld = 4096: 6.05 TB/s; with rows 128 KB apart at N = 8000, ld = 16064: 5.0 - 5.4 TB/s).  A 64-column
// strip never straddles a panel (4096 is a multiple of 64), so a kernel that walks a row strip by strip only needs the
// strip's column offset p_col(ld, j0) and the row stride p_lds(ld).  V, W and the mean keep the plain stride ld.
constexpr int PPW = 4096;
constexpr int RM_THREADS = 256;         // k_remove (ekf_remove.hip): threads per workgroup, one row each
constexpr int AQ_CHUNK = 64;            // k_assoc_query (ekf_associate.hip): landmarks per workgroup, one per lane of a wave
constexpr int JQ_TILE = 32;             // k_joint (ekf_joint.hip): rows / columns of a workgroup's tile of the sub-matrix
constexpr int JMAX = EKF_JMAX;          // landmarks per trajectory in one ekf_download_joint
constexpr int FB = 64;                  // ekf_factor (ekf_factor.hip): rows / columns of a block of the blocked Cholesky
constexpr int FACTOR_RHS = EKF_FACTOR_RHS;   // right-hand sides of one ekf_factor_solve / ekf_factor_multiply
// The rank fronts (ekf_rank_front.h): what a launch reads per trajectory of the BANK -- trajectories outside the call's range
// carry D = 0 -- is a row of ints {D, active bound, ...} and a row of doubles {..., gate, pad}; ekf_host_plan.h packs both
// (pack_direct / pack_linear) and lays them out in one buffer with the results (FrontTable).
// ekf_update_direct (k_direct, ekf_direct.hip): a trajectory brings up to MMAX fixes, at most one of them a pose fix of 3 rows:
// 3 + 2 (MMAX - 1) = 33 rows, 36 as whole k-tiles.  DIRECT_INTS ints {D, active bound, state index of row k (DIRECT_ROWS), 4 * fix +
// component of row k (DIRECT_ROWS)} and DIRECT_DBLS doubles {z (MMAX x 3), R (MMAX x 9, row-major 3 x 3 per fix), gate, pad}.
constexpr int DIRECT_ROWS = 36;
constexpr int DIRECT_INTS = 2 + 2 * DIRECT_ROWS;
constexpr int DIRECT_DBLS = MMAX * 12 + 2;
static_assert(3 + 2 * (MMAX - 1) <= DIRECT_ROWS && DIRECT_ROWS % 4 == 0 && DIRECT_ROWS <= KTOT, "a direct update's rows fit the pending ranks");
// ekf_update_linear (k_linear, ekf_linear.hip): a trajectory brings up to LINEAR_ROWS measurement rows over the pose and up to
// LINEAR_LMAX landmarks.  LINEAR_INTS ints {D, active bound (already raised over the sub-state), sub-state size ns, 0, state index
// of sub-state entry j (LINEAR_NS, -1 beyond ns)} and linear_dbls(dp, nsl) doubles packed by the launch's row cap dp and column
// count nsl = 3 + 2 * lstride: H (dp x nsl, row-major), r (dp), R (dp x dp, row-major, the upper triangle), gate, pad.
constexpr int LINEAR_LMAX = EKF_LINEAR_LMAX;
constexpr int LINEAR_ROWS = EKF_LINEAR_ROWS;
constexpr int LINEAR_NS = 3 + 2 * LINEAR_LMAX;
constexpr int LINEAR_INTS = 4 + LINEAR_NS + 1;
__host__ __device__ constexpr int linear_dbls(int dp, int nsl) { return dp * nsl + dp + dp * dp + 2; }
static_assert(LINEAR_NS <= DIRECT_ROWS && LINEAR_ROWS % 4 == 0 && LINEAR_ROWS <= KTOT && LINEAR_INTS % 2 == 0,
              "a linear update's rows fit the pending ranks");
// ekf_predict_linear (k_predict_pose, ekf_predict_linear.hip): one trajectory's record (host -> device, 192 B), for the
// trajectories [b0, b0 + count) of the call: the new pose mean, F = d(new pose)/d(old pose) row-major, Q row-major (the upper
// triangle is read), whether the trajectory takes part, and its active bound capped by its size (the host's: dso[b].neff may be
// stale behind an upload).
struct alignas(16) PredictIn {
  double pose[3];
  double F[9];
  double Q[9];
  int apply;
  int bound;
  double pad[2];
};
static_assert(sizeof(PredictIn) == 192, "PredictIn is 192 bytes");
// ekf_localize_* (k_loc_solve -> k_loc_rows, ekf_localize.hip): what one step's (one update pass's) sequential chain hands to
// the row kernel for one trajectory.  A column x_c = P(0..2, c), c >= 3, of the pose rows becomes
//     A x_c + sum_j B[j] [P(t[j], c); P(t[j] + 1, c)]       (A 3 x 3 and B[j] 3 x 2 row-major, j < m in observation order)
// below `bound`, the active bound of the step (the record's, raised to the handle's floor).  rej: bit j set = the NIS gate rejected
// observation j (B[j] = 0; the row kernel skips it); apply == 0: the step neither predicts nor observes -- nothing is touched.
constexpr int LOC_THREADS = 256;        // k_loc_rows: columns per workgroup
struct alignas(16) LocRec {
  double A[9];
  double B[MMAX][6];
  int t[MMAX];
  int m, bound;
  unsigned rej;
  int apply;
  double pad;
};
static_assert(sizeof(LocRec) == 928 && sizeof(LocRec) % 16 == 0, "LocRec is 928 bytes");
// ekf_hyp_* (ekf_hypotheses.hip): a bank of K pose hypotheses on ONE frozen map.  The map is a copy of a slot's stored triangle in
// the handle's layout (p_index / p_col / p_lds with the handle's ld) and of its mean; a hypothesis is this record plus its pose
// rows X[3][ldx] (P(r, c) at X[r * ldx + c], zero at and beyond its bound) and the LocRec its solve hands to its row launch.
// blk: the pose block's stored entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).  loglik: the sum over every observation the
// hypothesis has seen, gated out or not, of -1/2 (y^T S^-1 y + ln det S + 2 ln 2 pi) (terms that are not finite are left out,
// as evaluation.nis_consistency leaves them out); n_obs / n_rej count the observations and the gate's rejections.
struct alignas(16) HypState {
  double pose[3];
  double blk[6];
  double loglik;
  long long n_obs, n_rej;
  unsigned flags;
  int bound;
  double pad;
};
static_assert(sizeof(HypState) == 112, "HypState is 112 bytes");
__host__ __device__ constexpr int hyp_blk(int lo, int hi) { return 3 * lo - lo * (lo - 1) / 2 + (hi - lo); }
constexpr int HYP_THREADS = LOC_THREADS;   // k_hyp_rows / k_hyp_seed / k_hyp_reset / k_hyp_adopt: columns per workgroup
constexpr int HYP_CMP_THREADS = 256;       // k_hyp_compare: columns per workgroup, one row per blockIdx.y
// What the bank's launches take: the shared map (read only behind the seed), its mean, and the hypotheses' arrays.
struct HypView {
  const double* map; const double* mu; HypState* st; double* X; LocRec* rec;
  int n, ld, ldx, count;
};
// ekf_hypotheses_weigh / ekf_hypotheses_resample (k_hyp_weigh, k_hyp_plan, k_hyp_copy, k_hyp_split).  The header k_hyp_weigh
// leaves: top = the largest log-likelihood that weighs, sum / sum2 = the sums of w = exp(loglik - top) and of w^2, live = the
// hypotheses with w > 0, last = the last of them (-1: none), ess = sum^2 / sum2 and logmean = top + ln sum - ln K (0 and -inf in
// a degenerate bank: live == 0).  The launches behind it read the header on the device, so a resampling needs no host round trip.
constexpr int HYP_PLAN_THREADS = 1024;                 // k_hyp_weigh / k_hyp_plan: ONE workgroup, a chunk of ceil(K / 1024) <= 64 records per thread
constexpr int HYP_COPY_COLS = 2 * HYP_THREADS;         // k_hyp_copy / k_hyp_split: columns per workgroup, 16 bytes per lane and row
struct alignas(16) HypWeighOut {
  double top, sum, sum2, ess, logmean;
  int live, last;
  double pad;
};
static_assert(sizeof(HypWeighOut) == 64, "HypWeighOut is 64 bytes");
// head: the header; w: K weights (not normalised); anc / off: the plan (ancestors, offspring); exc: K ints of scratch, the
// exclusive scan of the surplus offspring (offspring - 1 of every survivor) the dead slots search
struct HypResampleView {
  HypWeighOut* head; double* w; int* anc; int* off; int* exc;
};
// ekf_hypotheses_mixture / ekf_hypotheses_run's log (k_hyp_mixture): the bank's pose mixture sum_k w_k N(pose_k, blk_k) behind k_hyp_weigh's
// header and weights -- the mean (the heading averaged on the circle), the covariance's stored entries in hyp_blk's order (the
// deviations' heading wrapped), the header's ess / logmean / live, best = the first hypothesis that weighs and whose loglik is
// the header's top (-1: none), and resampled = whether a resampling gated by ess_min acts on this header (hyp_gate_open).  A
// degenerate bank (live == 0): NaN mean and covariance, best = -1.
struct alignas(16) HypMixRow {
  double mean[3];
  double cov[6];
  double ess, logmean;
  int live, best, resampled, pad0;
  double pad;
};
static_assert(sizeof(HypMixRow) == 112, "HypMixRow is 112 bytes");
__host__ __device__ __forceinline__ int p_lds(int ld) { return ld < PPW ? ld : PPW; }
__host__ __device__ __forceinline__ long p_col(int ld, int j) { return (long)(j >> 12) * ((long)ld * PPW) + (j & (PPW - 1)); }
// the same as a 32-bit byte offset (ekf_create bounds one covariance by 4 GiB)
__host__ __device__ __forceinline__ unsigned p_col8(int ld, unsigned j) { return (j >> 12) * ((unsigned)ld * (unsigned)(PPW * 8)) + (j & (unsigned)(PPW - 1)) * 8u; }
__host__ __device__ __forceinline__ long p_index(int ld, int i, int j) { return p_col(ld, j) + (long)i * p_lds(ld); }
// panels / doubles allocated per trajectory (every panel keeps all `rows` rows: downloads and the dense product get the
// mirrored matrix in place)
__host__ __device__ __forceinline__ int p_panels(int ld) { return ld <= PPW ? 1 : (ld + PPW - 1) / PPW; }
__host__ __device__ __forceinline__ long p_alloc(int rows, int ld) { return ld <= PPW ? (long)rows * ld : (long)p_panels(ld) * rows * PPW; }

constexpr int FLAG_PREDICT = 1;         // StepIn.flags
constexpr int FLAG_UPDATE = 2;

// One step's inputs for one trajectory (host -> device, 352 B).
struct StepIn {
  double lin, ang;
  int m;
  int flags;
  int neff;             // active bound: state indices >= neff have never been correlated with anything
  int pad;
  int idx[MMAX];
  double range[MMAX];
  double bearing[MMAX];
};

// k_hyp_score (ekf_hyp_assoc.hip): one workgroup of HS_WAVES waves per hypothesis, lane = landmark within a chunk of HS_CHUNK.
// Where it writes.  Query mode (cand set; step nullptr): ekf_associate's outputs with stride = m for the hypotheses of the
// launch's range, row = hypothesis - k0 -- cand_nis / cand_logdet / min_nis may be nullptr, all_nis / all_logdet come together
// or not at all with `cap` landmarks per row.  Step mode (step set; cand nullptr): hypothesis k's record step[k] and assignment
// row assign[k * MMAX ..], indexed by the hypothesis itself; accept: the NIS an observation's candidate must not exceed, miss:
// the log-likelihood every dropped observation adds to the hypothesis.
constexpr int HS_WAVES = 4;
constexpr int HS_CHUNK = 64;
struct HypScoreOut {
  int* cand; double *cand_nis, *cand_logdet, *min_nis, *all_nis, *all_logdet; int cap;
  StepIn* step; int* assign; double accept, miss;
};

// What one sequential iteration (one observed landmark j, src/replay_no_ros.py:436-480) hands to
// the panel kernel, expressed on the compressed index set C.  Pairs are stored adjacent so that a
// single 16-byte LDS broadcast read fetches both rows of a 2-row quantity.
struct alignas(16) SolveIter {
  double h5t[5][2];     // {H[0][k], H[1][k]}: the 2x5 Jacobian on {0,1,2,t_j,t_j+1}    (:466-469)
  double si[4];         // S_j^{-1} row-major                                             (:473)
  double y[2];          // innovation                                                     (:455-458)
  double kc[CMAX][2];   // K_j[C[a],:]                 (0 for a >= c)
};
static_assert(sizeof(SolveIter) % 16 == 0, "SolveIter must stay 16-byte granular");

// The pending factors restricted to C, written by the solve kernel for the panel kernel's scalar loads:
// per trajectory  facW[a][k] = W[C[a]][k]  then  facV[a][k] = V[k][C[a]],  both [CMAX][KTOT], zero-filled
// up to the next multiple of 8 ranks.
constexpr int FACS = 2 * CMAX * KTOT;

// Output of the sequential compressed solve for one trajectory; read by the panel and pass kernels.
struct alignas(16) SolveHead {
  double g[2];          // G[0,2], G[1,2] of the motion Jacobian (0 when prediction is off)
  double rd[3];         // motion noise added to the pose block (0 when prediction is off)
  double p22h;          // 0.5 * P[2,2] before the step
  double dacc_old[3];   // pose-block noise already pending before this step
  int cmax;             // largest gathered state index (panel waves starting beyond it never read W)
  unsigned rej;         // NIS gate (ekf_set_nis_gate): bit j set = landmark j of this pass was rejected (its record is zero)
  int c;                // 3 + 2m
  int m;
  int kbase;            // ranks pending before this step (multiple of 4)
  int neff;             // active bound of this step (rows/cols >= neff of P are untouched diagonal)
  int C[CMAX + 1];      // gathered state indices, padded with 0
  double prow[2][CMAX + 1];   // P(0, C[a]) and P(1, C[a]) before the step (what state indices 0,1 gather)
};
struct alignas(16) SolveOut : SolveHead {
  SolveIter it[MMAX];
};
static_assert(sizeof(SolveHead) % 16 == 0, "SolveHead must stay 16-byte granular");
// (SolveOut = head, then the records: `it` starts at sizeof(SolveHead))

// ---- fused cadence (ekf_cadence.hip): everything between two covariance passes of an uploaded stream as ONE solve launch
// and ONE panel launch.  Right after a pass nothing is pending and the stream knows the next landmark indices: the union
// panel P(C_u, i), C_u = {0,1,2} + the landmark indices of all updates up to the next pass, is gathered from P_base once, the
// predictions and the sequential landmark updates of src/replay_no_ros.py:368-480 are replayed on it, and all ranks are
// appended at once.
// Round 5: the cadence is PACKED.  A trajectory's stream is the flat sequence  P_t, L_t,0 .. L_t,m_t-1, P_t+1, ...  (P = the
// prediction of step t, L = one landmark update); a cadence takes the next <= CAD_SLOTS landmark updates of that sequence,
// whatever steps they belong to (a step may be cut: its remaining landmarks open the next cadence, without a second
// prediction), plus every prediction in between -- exactly 2 ranks per landmark update, no rounding of a step's landmark
// count to a slot size, steps that observe nothing ride along for free.  Every trajectory of a bank walks its OWN sequence
// (trajectories are closed systems, src/replay_no_ros.py:269-482 couples nothing): after a pass each one has used its 40
// slots, however its landmark counts wander (CadPlan, planned on the host: ekf_host_plan.h).
// Slots are RIGHT-ALIGNED: a cadence of `nslots` updates uses the slots s0 = CAD_SLOTS - nslots .. CAD_SLOTS - 1; slot s sits
// at positions pa(s), pa(s) + 1 of C_u with pa(s) = 3 + 2 (CAD_SLOTS - 1 - s): later slots at LOWER positions, the last one
// always at 3, 4 -- "everything a later update still needs" is always the prefix [0, pa(s)) of the positions: compile-time
// bounds for the panel's register array, a shrinking prefix of lanes for the solve, and a short cadence costs what its
// slots cost.  A landmark observed twice has two slots (duplicate positions carry identical values); positions beyond
// 3 + 2 nslots gather index 0 and are never read.
constexpr int CAD_SLOTS = KTOT / 2;                  // landmark slots of a cadence (2 ranks each)
constexpr int CAD_CU = 3 + 2 * CAD_SLOTS;            // gathered positions at most (83)
__host__ __device__ constexpr int cad_pa(int s) { return 3 + 2 * (CAD_SLOTS - 1 - s); }
// record of slot s (doubles): h5t[5][2], si[4], y[2], then K_s[C_u[a], :] for the positions a < pa(s) a later slot or
// step still reads; records are packed back to back
__host__ __device__ constexpr int cad_rec_off(int s) { return 16 * s + 2 * (s * (3 + 2 * (CAD_SLOTS - 1)) - s * (s - 1)); }
struct CadGeom {
  static constexpr int GM = CAD_SLOTS;               // landmark slots
  static constexpr int CU = CAD_CU;                  // gathered positions
  __host__ __device__ static constexpr int pa(int s) { return cad_pa(s); }
  __host__ __device__ static constexpr int rec_off(int s) { return cad_rec_off(s); }
  static constexpr int REC = cad_rec_off(CAD_SLOTS);
};
constexpr int CAD_REC_MAX = CadGeom::REC;            // 4000 doubles
// What one trajectory does in one cadence (host -> device, 32 B): the steps t0 .. t0 + ns - 1 of the uploaded stream; of the
// first one the landmarks from j0 on (j0 > 0: the step was cut by the previous cadence, its prediction has happened), of
// the last one the landmarks up to jend (exclusive; the rest open the next cadence).  ns == 0: nothing (the trajectory has
// reached the end of the range; its ranks of this cadence are zero).
struct CadPlan {
  int t0, j0, ns, jend;
  int nslots;                 // landmark updates (<= CAD_SLOTS)
  int neff;                   // active bound of the cadence (its last step's, raised to the handle's floor)
  int pad[2];
};
struct alignas(16) CadHead {
  int nslots;                 // landmark slots in use: CAD_SLOTS - nslots .. CAD_SLOTS - 1
  int neff;                   // active bound of the cadence
  int npred;                  // steps touched (a prediction each, except a first step cut by the previous cadence)
  int pad0;
  int sfirst[CAD_SLOTS];      // slot of the first landmark of touched step p, or of the next one that has any (CAD_SLOTS: none)
  int C[CAD_CU + 1];          // gathered state indices by position
  double g[CAD_SLOTS][2];     // G[0,2], G[1,2] of touched step p's motion Jacobian (0 when it predicts nothing)
  double prow[2][CAD_CU + 1]; // (diagnostic) P(0, C_u[a]), P(1, C_u[a]) before the cadence
  double ddpose[2][4];        // what the cadence's predictions add to P_base(0, l), P_base(1, l), l < 3 (the pose block)
  double rdsum[4];            // pose-block noise of the cadence's predictions (applied by the panel launch when no rank is pending)
};
struct alignas(16) CadOut : CadHead {
  double rec[CAD_REC_MAX];
  double posevw[CAD_SLOTS][3][4];   // the new ranks' entries at the pose's state indices l < 3: V[2s][l], V[2s+1][l], W[l][2s], W[l][2s+1]
  double posefin[4][4];             // (k_solve_cad<true>: chained runs) the pose block P(l, l') after the cadence, motion noise included
  unsigned long long rej;           // (NIS gate on) bit s set = slot s was rejected: its record and posevw entries are zero
  unsigned long long pad1[3];       // (CadOut stays 32-byte granular)
};
// (chained runs) a cadence's inputs as k_solve_cad needs them -- positions, per-step counts and slots, motion inputs,
// measurements -- formed ONE CADENCE AHEAD by an otherwise idle workgroup of the chain launch (cad_positions is two dependent
// memory round trips: 2.5 us at the head of the solve, of the chain launch and of its gather workgroups)
struct alignas(16) CadPre {
  int nslots, pad[3];
  int C[128];                                // gathered state indices by position (0 beyond the cadence's)
  int cnt[CAD_SLOTS + 4], first[CAD_SLOTS + 4], lo[CAD_SLOTS + 4];   // per touched step: landmarks, slots in front of it, first landmark
  int fl[CAD_SLOTS];                         // per touched step: StepIn.flags (a first step cut by the previous cadence: no prediction)
  double la[CAD_SLOTS][2];                   // per touched step: (lin, ang)
  double z[CAD_SLOTS][2];                    // per slot: (range, bearing)
};
static_assert(sizeof(CadPre) % 16 == 0, "CadPre must stay 16-byte granular");
static_assert(sizeof(CadHead) % 16 == 0, "CadHead must stay 16-byte granular");
static_assert(sizeof(CadPlan) == 32, "CadPlan is 32 bytes");

// Device-side association: one window of raw AprilTag detections per trajectory.
constexpr int DMAX = EKF_DMAX;          // detections per window (256)
constexpr int AMAX = EKF_AMAX;          // distinct tags per window (32: two update passes of MMAX landmarks)
constexpr int TAGMAX = 1024;            // tag ids [0, TAGMAX) (tag36h11 has 587)
constexpr int IGNMAX = 16;

struct DetIn {                          // host -> device
  double lin, ang;
  int count;
  int pad;
  int tag_id[DMAX];
  double pose_err[DMAX];
  double pose_t[DMAX][3];
};

struct AssocOut {                       // what the reference returns as tags_positions (:331-337), update order
  int m;
  int n_after;
  int idx[AMAX];
  int tag_id[AMAX];
  double xw[AMAX], yw[AMAX], err[AMAX], range[AMAX], bearing[AMAX];
};

// ekf_localize_detections (k_loc_associate, ekf_loc_assoc.hip): the tags of a trajectory's last localisation window that its frozen
// map does not hold -- `total` distinct ids, the first AMAX of them in order of first appearance (-1 beyond).
struct LocUnmatched {
  int total;
  int pad;
  int tag_id[AMAX];
};

struct AssocConfig {
  double gate2;                         // 1.5^2 (:289)
  double init_var;                      // 1e4   (:356-357)
  int n_ignore;
  int active_bound;
  int ignore[IGNMAX];                   // IGNORE_TAGS (:36, :286)
};

// The innovation log (ekf_log_innovations): a device ring of `cap` step rows, each batch x AMAX entries (landmark index, y, S,
// NIS: ekf_innovations.hip) plus batch counts.  InnovLog names where a launch writes: its step t goes to ring row
// (slot0 + t) % cap -- a one-step launch has t = 0 -- at positions jbase + j (jbase = 16 p for update pass p of a step).
struct alignas(16) InnovRec {
  double y[2];
  double S[4];          // row-major
  double nis;
  int idx;
  int rejected;         // NIS gate: 1 = the update was rejected (the solve's decision, copied), 0 = applied
};
static_assert(sizeof(InnovRec) == 64, "InnovRec is 64 bytes");
struct InnovLog {
  InnovRec* rec;        // [cap][batch][AMAX]
  int* m;               // [cap][batch]: landmark updates each step applied (more than AMAX: only the first AMAX are kept)
  long slot0;
  int cap, jbase;
};
// The pose log (ekf_log_poses): a device ring of `cap` step rows, each batch x POSE_ROW doubles: the pose mean x, y, theta and
// the pose block P[0:3, 0:3] row-major, as they stand after the step.  PoseLog names where a launch writes: its step t goes to
// ring row (slot0 + t) % cap -- a one-step launch has t = 0.  row == nullptr: the launch logs no pose.
constexpr int POSE_ROW = 12;
struct PoseLog {
  double* row;          // [cap][batch][POSE_ROW]
  long slot0;
  int cap;
};
// What a read-only query reads of the filter (ekf_api.hip: pending_view; the launchers of k_marginals, k_assoc_query, k_joint):
// P_base, the kb pending ranks, pose noise, mean, sizes and last solve's records of trajectories [b0, b0 + count).
struct PendingView {
  const double *P, *V, *W, *dacc, *mu;
  const int* nact;
  const SolveOut* so;
  int ld; long pstride; int b0, count, kb;
};
// The factor workspace of ekf_factor (ekf_factor.hip): per factored trajectory lw x lw doubles, row-major, tstride apart; the
// status words {info, n, nblk, 0} and the log-determinant of each.
struct FactorView {
  double* ws; size_t tstride; int lw; int* fstat; double* flog;
};
// What the launches that move the filter take of a handle, the same for every launch of a call (ekf_api.hip: bank_view; the
// launchers of ekf_launch.h unpack it into their kernel's arguments): P_base, the rank slots, sizes, last solve's records,
// sticky flags, the pass's work-queue words and the layout of the whole bank.
struct BankView {
  double *P, *V, *W; int* nact; SolveOut* so; unsigned *flags, *queue;
  int ld; long pstride; int batch;
};
// The halves of the double-buffered arrays one launch reads and writes (ekf_api.hip: step_bufs, which says which copy holds
// what): mean and pending pose noise in and out; for a cadence's launches also its records and the two copies of the pose rows,
// as they stood before the cadence (prow3_in) and as its panel launch leaves them (prow3_out).
struct StepBufs {
  const double* mu_in; double* mu_out; const double* dacc_in; double* dacc_out; CadOut* cad;
  double *prow3_in, *prow3_out;         // (prow3_in is written once per chained run: launch_snap_pose)
};
// y^T S^-1 y with S^-1 = [[a, b], [c, d]]
__host__ __device__ __forceinline__ double innov_nis(double y0, double y1, double a, double b, double c, double d) {
  return y0 * (a * y0 + b * y1) + y1 * (c * y0 + d * y1);
}

// The NIS validation gate (ekf_set_nis_gate): landmark update j is rejected -- its mean, covariance and ranks untouched --
// when NIS = y^T S^-1 y exceeds the threshold.  Every wave that acts on the decision forms it itself from the same y and S^-1
// with this one expression (a NaN NIS is never rejected).
__host__ __device__ __forceinline__ bool innov_reject(double y0, double y1, double a, double b, double c, double d, double gate) {
  return innov_nis(y0, y1, a, b, c, d) > gate;
}

struct DeviceConfig {
  double rd[3];         // diag of R  (src/replay_no_ros.py:421)
  double qd[2];         // diag of Q  (:438)
  double arc_threshold; // :376
  int enable_measurement_model, enable_circular_interpolation, disable_motion_model;
  double nis_gate;                      // NIS gate threshold (ekf_set_nis_gate; read only while gate_rej is set)
  unsigned long long* gate_rej;         // per trajectory: updates the gate rejected; nullptr = the gate is off
  const double* noise;                  // per trajectory (ekf_set_noise): NOISE_ROW doubles {rd0, rd1, rd2, qd0, qd1};
                                        // nullptr = rd / qd above for every trajectory
};

// Trajectory b's noise constants (ekf_set_noise).  NZ: the instantiations launched while the handle's table is set
// (cfg.noise != nullptr); the others never call this and read cfg.rd / cfg.qd at their sites as they always have.
constexpr int NOISE_ROW = 5;
struct NoiseRow {
  double rd[3], qd[2];
};
__device__ __forceinline__ NoiseRow noise_row(const DeviceConfig& cfg, int b) {
  const double* r = cfg.noise + (long)NOISE_ROW * b;
  return NoiseRow{{r[0], r[1], r[2]}, {r[3], r[4]}};
}

}  // namespace ekf
