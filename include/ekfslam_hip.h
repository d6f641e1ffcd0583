/*
 * ekfslam_hip.h -- C ABI of libekfslam_hip.so: the MI355X (gfx950) EKF-SLAM predict/update core.
 *
 * The reference (AHHHZ975/SLAM-Duckietown) has no FFI layer: its hot path is one Python
 * function, EKF_pose_estimation (src/replay_no_ros.py:269-482), and src/ekf_bindings.py is an
 * empty placeholder for "EKF bindings".  This header is what that placeholder would bind with
 * ctypes.  Each entry point names the reference lines it replaces.  Plain pointers and sizes
 * only; every function returns an int status (0 = EKF_OK) unless stated otherwise.
 *
 * State layout at this boundary is the reference's own (src/replay_no_ros.py:69-70, :341-360):
 *   mu : (n,)   float64   [x, y, theta, l0x, l0y, ..., l(N-1)x, l(N-1)y],  n = 3 + 2N
 *   P  : (n,n)  float64   row-major (NumPy C order)
 * On the device a covariance is kept as its upper triangle, row-major with a padded row stride up to n_max = 4096 and in
 * column panels of 4096 doubles beyond (every row segment of a tile 32 KB from the next, whatever the size of the state);
 * uploads and downloads translate -- the layout never shows at this boundary.
 * Device buffers are owned by the handle; host arrays are borrowed for the duration of a call.
 * A handle is not thread-safe: one handle per device per host thread.
 */
#ifndef EKFSLAM_HIP_H
#define EKFSLAM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EKF_OK 0
#define EKF_ERR_ARG (-1)      /* bad argument (message in ekf_last_error) */
#define EKF_ERR_HIP (-2)      /* a HIP runtime call failed, or no gfx950 device */
#define EKF_ERR_STATE (-3)    /* call not valid in the current state */

#define EKF_MMAX 16           /* max landmarks per single device update pass (longer lists are split) */
#define EKF_N_MAX_LIMIT 21823 /* largest n_max = 3 + 2N ekf_create accepts (N = 10910): the kernels address one
                                 covariance with unsigned 32-bit byte offsets, so what is allocated for it -- rows
                                 (n_max rounded up to 64) x column panels of 4096 doubles, 8 bytes each -- must
                                 stay below 4 GiB; larger values fail with EKF_ERR_ARG */

/* sticky per-trajectory flags, ekf_status_flags() */
#define EKF_FLAG_NONFINITE 1u /* a non-finite mean entry was produced (q = 0 at :466-469, singular S at :473) */
#define EKF_FLAG_INTERNAL 4u  /* a bounded wait inside a single-launch step timed out (the GPU did not run the solve
                                 workgroup of the launch beside its panel workgroups for tens of ms).  A timed-out
                                 wave writes nothing while other waves of the same step may have written: the
                                 trajectory's state is UNDEFINED from there on, and ekf_sync and every ekf_download_*
                                 (state, mean, block, tags, tag index) return EKF_ERR_STATE while the flag is set.  The
                                 same status is returned, for every trajectory of the handle, after an enqueueing call
                                 failed half way.  Recovery: upload the trajectory again (ekf_upload_state* clears the
                                 condition); ekf_set_option("fused_step", 0) selects the two-launch step, which has no wait. */
#define EKF_FLAG_ASSOC 2u     /* device-side association dropped a detection: tag id outside [0, 1024), state full,
                                 or more than EKF_AMAX distinct tags in one window */
#define EKF_DMAX 256          /* detections per window for ekf_step_detections (the reference's normal mode: a 0.7 s window
                                 of every camera frame, src/replay_no_ros.py:17 -- 21 frames x a dozen tags) */
#define EKF_JMAX 64           /* landmarks per trajectory in one ekf_download_joint (sub-state of up to 3 + 2*64 = 131) */
#define EKF_LINEAR_LMAX 16   /* landmarks in the sub-state of one ekf_update_linear: ns <= 3 + 2*16 = 35 */
#define EKF_LINEAR_ROWS 32   /* measurement rows D per trajectory of one ekf_update_linear (whole k-tiles of 4) */
#define EKF_AMAX 32           /* distinct tags per window the device-side association takes (two update passes of EKF_MMAX) */

typedef struct ekf_handle ekf_handle;

/* Module constants of src/replay_no_ros.py:15-31 and the literals at :289, :356, :376. */
typedef struct ekf_config {
  double motion_sigma;                /* MOTION_MODEL_VARIANCE       (:15)  default 0.1  */
  double meas_sigma;                  /* MEASUREMENT_MODEL_VARIANCE  (:16)  default 0.7  */
  double arc_threshold;               /* |ang| <= thr -> straight branch (:376) default 1e-2 */
  double landmark_init_var;           /* new-landmark variance (:356-357)   default 1e4  */
  int enable_measurement_model;       /* (:18)  default 1 */
  int enable_circular_interpolation;  /* (:19)  default 1 */
  int disable_motion_model;           /* (:28)  default 0 */
  int reserved;
} ekf_config;

int ekf_config_default(ekf_config *cfg);

/* Number of HIP devices visible to the process (0, and EKF_OK, when there is none). */
int ekf_device_count(int *count);

/* Create a filter bank of `batch` independent trajectories on HIP device `device`, each with room
 * for n_max = 3 + 2*N_max states.  All trajectories start as the reference does
 * (src/replay_no_ros.py:69-70): n = 3, mu = 0, P = motion_sigma * I3.  Fails (EKF_ERR_HIP) when no
 * gfx950 device is present: there is no CPU fallback. */
int ekf_create(int device, int n_max, int batch, const ekf_config *cfg, ekf_handle **out);
int ekf_destroy(ekf_handle *h);

/* Whole state in / out for trajectory b (checkpoint, parity checks).  Blocking.
 * A covariance is symmetric: the device keeps its upper triangle only, so of an uploaded P the upper
 * triangle is authoritative (entries below the diagonal are not even sent: 56 % of the matrix crosses PCIe
 * at n = 4003), and a download returns that triangle mirrored (the reference's own Sigma is symmetric to
 * rounding). */
int ekf_upload_state(ekf_handle *h, int b, const double *mu, const double *P, int n);
int ekf_upload_state_diag(ekf_handle *h, int b, const double *mu, const double *diagP, int n);
int ekf_download_state(ekf_handle *h, int b, double *mu, double *P, int n);
int ekf_download_mean(ekf_handle *h, int b, double *mu, int n);
/* rows [r0, r0+rows) x cols [c0, c0+cols) of the covariance into out (row-major rows x cols), e.g. the 3x3
 * pose block for consistency statistics without shipping n^2 doubles.  Flushes the pending update. */
int ekf_download_block(ekf_handle *h, int b, int r0, int c0, int rows, int cols, double *out);
/* Marginal covariances of trajectories [b0, b0+count) without applying the pending update: pose (count x 9: the 3x3
 * pose block, row-major) and, if landmarks != NULL, every landmark's 2x2 block (count x cap x 4, row-major; blocks
 * beyond a trajectory's landmark count are NaN); n_landmarks (may be NULL) receives each count.  For NEES at every
 * step, the ellipses of a plot, a pose covariance to publish: one kernel reads P_base at the blocks and the W rows / V
 * columns of their indices over the pending ranks -- O(n k) per trajectory -- and writes pinned destinations (e.g.
 * from ekf_host_alloc) directly, anything else through one copy.
 * Blocking, and stream-ordered behind everything enqueued.  It runs no covariance pass and no mirror, and changes
 * nothing that decides later scheduling: after the call the same calls give bit-identical results and the same
 * ekf_debug_cadences / ekf_debug_chained / ekf_debug_lookaheads / ekf_profile_passes counts as without it.  The
 * result equals a flushed ekf_download_block to rounding (the pending ranks are summed in another order), and is
 * bit-identical where nothing is pending.  Valid on every path: per-step kernels, single-launch steps, fused cadences
 * ended mid-cadence, chained and look-ahead runs, the small-state path.  Device-side sizes are refreshed first.
 * EKF_ERR_ARG for a bad range, NULL pose, or cap below the largest landmark count in the range; EKF_ERR_STATE if a
 * trajectory of the range carries EKF_FLAG_INTERNAL or an earlier call failed half way (as the other downloads). */
int ekf_download_marginals(ekf_handle *h, int b0, int count, double *pose, double *landmarks, int cap,
                           int *n_landmarks);
/* Likelihood association of UNLABELLED observations: trajectories [b0, b0+count) each bring m[b] <= stride <= EKF_MMAX
 * range/bearing observations (range, bearing: count x stride) and every landmark l of the trajectory's map is scored against
 * every observation q on the device.  Per landmark, once: the current joint 5x5 covariance of (pose, landmark l) -- P_base plus
 * the pending ranks, read with ekf_download_marginals' bounds, no covariance pass --, the measurement model at the current mean
 * (what ekf_download_mean returns), S = H P5 H^T + Q_b with the measurement noise in effect for the trajectory (ekf_set_noise's
 * row if set, else the handle's), S^-1 and ln det S.  Per observation: y = z - z^ (bearing wrapped), NIS = y^T S^-1 y -- the
 * quantity of the innovation log and the NIS gate -- and the ranking score d = NIS + ln det S (the negative log-likelihood up
 * to constants; plain NIS would always prefer the most uncertain landmark).
 * cand (count x stride x 2) receives the landmarks of the two smallest d, cand_nis and cand_logdet (same shape, may be NULL)
 * their NIS and ln det S, min_nis (count x stride, may be NULL) the smallest NIS over ALL landmarks ("does this observation fit
 * nothing?").  The reduction is deterministic: ties go to the lower index, a NaN score never wins; a trajectory without
 * landmarks or whose scores are all NaN, and the rows q >= m[b], get index -1 and NaN.  all_nis and all_logdet (count x
 * stride x cap, both or neither, may be NULL) receive the full matrices; entries beyond a trajectory's landmark count are NaN.
 * Pinned destinations (e.g. from ekf_host_alloc) are written directly, anything else through one copy.
 * Blocking, and stream-ordered behind everything enqueued.  It runs no covariance pass, and changes nothing that decides
 * later scheduling: after the call the same calls give bit-identical results and the same ekf_debug_cadences /
 * ekf_debug_chained / ekf_debug_lookaheads / ekf_profile_passes counts as without it.  Valid on every path: per-step kernels,
 * single-launch steps, fused cadences ended mid-cadence, chained and look-ahead runs, the small-state path.  Device-side sizes
 * are refreshed first.
 * EKF_ERR_ARG for a bad trajectory range, stride outside 1..EKF_MMAX, m[b] outside 0..stride, a non-finite observation, NULL
 * cand, or all_* given with cap below the largest landmark count of the range; EKF_ERR_STATE if a trajectory of the range
 * carries EKF_FLAG_INTERNAL or an earlier call failed half way (as the other downloads). */
int ekf_associate(ekf_handle *h, int b0, int count, const double *range, const double *bearing, const int *m, int stride,
                  int *cand, double *cand_nis, double *cand_logdet, double *min_nis, double *all_nis, double *all_logdet, int cap);
/* Joint covariance (and mean) of the pose and a chosen SUBSET of landmarks, cross-covariances included, without applying the
 * pending update: what joint-compatibility association, a submap hand-off or the separation of two landmarks need, and what
 * otherwise takes ekf_flush + ekf_download_block per block pair.  Trajectories [b0, b0+count) each name k[bi] <= stride <=
 * EKF_JMAX landmarks in landmarks[bi*stride + 0..k[bi]), in any order; the sub-state of trajectory bi is [x, y, theta,
 * l_j0 x, l_j0 y, l_j1 x, ...] in the order given, ns = 3 + 2*stride.  cov (count x ns x ns, row-major) receives the CURRENT
 * covariance of that sub-state -- P_base plus the pending ranks plus the pending pose noise, read with
 * ekf_download_marginals' bounds --, mean (count x ns, may be NULL) its mean, bit for bit what ekf_download_mean returns at
 * those indices.  Rows and columns beyond 3 + 2*k[bi] are NaN in both; k[bi] = 0 returns the pose alone.
 * Every entry is formed once, from the stored upper triangle (the smaller state index as the row), and mirrored: cov is
 * exactly symmetric.  The ranks of an entry are summed in a fixed order that does not depend on the selection: a permuted
 * selection gives the permuted result bit for bit, a subset the corresponding entries of a superset bit for bit, and where
 * nothing is pending the result is the stored value bit for bit; against a flushed download it is equal to rounding (the
 * ranks are summed in another order).
 * One gather kernel (a workgroup per trajectory and 32 x 32 tile of the sub-matrix) writes pinned destinations (e.g. from
 * ekf_host_alloc) directly, anything else through a staging buffer of the handle and one copy.
 * Blocking, and stream-ordered behind everything enqueued.  It runs no covariance pass and no mirror, writes nothing the
 * filter owns and changes nothing that decides later scheduling: after the call the same calls give bit-identical results
 * and the same ekf_debug_cadences / ekf_debug_chained / ekf_debug_lookaheads / ekf_profile_passes counts as without it.
 * Valid on every path: per-step kernels, single-launch steps, fused cadences ended mid-cadence, chained and look-ahead runs,
 * the small-state path.  Device-side sizes are refreshed first.
 * EKF_ERR_ARG (nothing changed, the handle usable) for a bad trajectory range, stride outside 1..EKF_JMAX, k[bi] outside
 * 0..stride, a landmark index outside the trajectory's map or named twice in one trajectory, NULL landmarks, k or cov;
 * EKF_ERR_STATE if a trajectory of the range carries EKF_FLAG_INTERNAL or an earlier call failed half way (as the other
 * downloads). */
int ekf_download_joint(ekf_handle *h, int b0, int count, const int *landmarks, const int *k, int stride,
                       double *mean, double *cov);
/* The Cholesky factor of the WHOLE covariance, on the device: ekf_factor computes U, upper triangular with a positive
 * diagonal and P = U^T U, for trajectories [b0, b0+count) -- what full-state NEES e^T P^-1 e, the question "is P still a
 * covariance?" (every update here is P -= K S K^T, not the Joseph form), the entropy of the map (ln det P) and posterior
 * draws (a square root of P) need, without covariance(b) and a host factorisation per trajectory.  P is the current
 * covariance: the pending update is applied first (a pass the caller pays for, as ekf_download_block does) and device-side
 * sizes are refreshed; the filter's own state is never written -- U goes into a workspace of the handle (per trajectory the
 * square of the range's largest n rounded up to 64, 8 bytes each: 130 MB at n = 4003), and afterwards the filter is bit for
 * bit where a plain ekf_flush at that point would have left it.  A right-looking blocked factorisation, block 64; the rank-64
 * down-dates of the trailing triangle run on the fp64 matrix cores; the reduction order is fixed, so a trajectory's U is
 * bit-identical across repeats, bank positions and ranges.
 * logdet[bi] = 2 sum_i ln u_ii.  info[bi] follows LAPACK dpotrf: 0 = positive definite, i > 0 = the leading minor of order i is
 * not (the first pivot that is <= 0 or not finite, 1-based); such a trajectory gets logdet = NaN, does not disturb the others
 * and sets no sticky flag (this is a query).  Either output may be NULL.  Blocking, and stream-ordered behind everything
 * enqueued.
 * The factor is a SNAPSHOT: it stays -- with the range and each trajectory's n at that time -- until the next ekf_factor,
 * ekf_factor_release or ekf_destroy; later filter calls neither change nor invalidate it.
 * ekf_factor_solve: rhs is count x nrhs x stride (nrhs in 1..EKF_FACTOR_RHS, stride >= the largest factored n of the range;
 * a trajectory reads the first n entries of each column); white (same shape) = U^-T rhs, entries beyond a trajectory's n NaN;
 * quad (count x nrhs) = |white|^2 = rhs^T P^-1 rhs.  Either output may be NULL, not both.
 * ekf_factor_multiply: out = U^T z, same shapes: cov(out) = P for z ~ N(0, I).
 * ekf_download_factor: U of trajectory b as n x n row-major, zeros below the diagonal.
 * Every output of a trajectory whose info != 0 is NaN, and ekf_download_factor returns EKF_ERR_STATE for it.
 * EKF_ERR_ARG, with nothing changed: a bad range, NULLs, nrhs or stride out of bounds, a non-finite rhs or z, n different from
 * the factored n.  EKF_ERR_STATE: no factor held, a range outside the factored one; for ekf_factor a trajectory of the range
 * carries EKF_FLAG_INTERNAL or an earlier call failed half way (as the downloads).  EKF_ERR_HIP: the workspace cannot be
 * allocated (the message carries the byte count); any previous factor is released and the handle stays usable. */
#define EKF_FACTOR_RHS 16     /* right-hand sides of one ekf_factor_solve / ekf_factor_multiply */
int ekf_factor(ekf_handle *h, int b0, int count, double *logdet, int *info);
int ekf_factor_solve(ekf_handle *h, int b0, int count, const double *rhs, int nrhs, int stride,
                     double *white, double *quad);
int ekf_factor_multiply(ekf_handle *h, int b0, int count, const double *z, int nrhs, int stride, double *out);
int ekf_download_factor(ekf_handle *h, int b, double *U, int n);
int ekf_factor_release(ekf_handle *h);
int ekf_state_size(ekf_handle *h, int b, int *n);

/* Innovation log: every landmark update's landmark index, innovation y (2), innovation covariance S (2x2, row-major) and
 * NIS = y^T S^-1 y -- the consistency check that needs no ground truth; the sum of -(NIS + log det 2 pi S) / 2 over a run is
 * its log-likelihood (how MOTION_MODEL_VARIANCE / MEASUREMENT_MODEL_VARIANCE, src/replay_no_ros.py:15-16, are tuned).  Off by
 * default.  The log is a device ring of the last `capacity` logged steps, EKF_AMAX entries per step and trajectory, filled on
 * every path that applies landmark updates (per-step kernels, single-launch steps, fused cadences, chained and look-ahead
 * runs, the small-state path); switching it on or off changes nothing about the filter (same bits, same scheduling and
 * counters).  A logged STEP is one call of ekf_update, ekf_step, ekf_step_fetch or ekf_step_detections, or one stream step
 * ekf_stream_run runs (a lone ekf_predict is not one); each trajectory writes its own column of a step row.  A step's m is the
 * number of updates it applied, in application order: both update passes of a step with more than EKF_MMAX landmarks, the
 * device association's order (ekf_download_tags), and a stream step cut by a cadence boundary all count as one step.  A
 * step that applies more than EKF_AMAX updates keeps the first EKF_AMAX and reports its true m.
 * ekf_log_innovations: capacity > 0 allocates the ring (capacity x batch x EKF_AMAX entries) and restarts the count at 0;
 * 0 switches the log off and frees it (after a stream synchronisation).
 * ekf_innovation_steps: steps logged since the log was switched on.
 * ekf_download_innovations: steps [first, first + count) into m (count x batch), idx (count x batch x EKF_AMAX), y (x 2),
 * S (x 4) and nis (x 1); idx, y, S and nis may be NULL.  Entries beyond a step's m are -1 / NaN.  Blocking and
 * stream-ordered behind everything enqueued; runs no covariance pass or mirror and changes nothing that decides later
 * scheduling.  EKF_ERR_ARG if the range is not inside the last `capacity` logged steps, EKF_ERR_STATE with the log off or
 * under EKF_FLAG_INTERNAL (as the other downloads). */
int ekf_log_innovations(ekf_handle *h, int capacity);
int ekf_innovation_steps(ekf_handle *h, long long *logged);
int ekf_download_innovations(ekf_handle *h, long long first, int count, int *m, int *idx, double *y, double *S, double *nis);

/* Pose log: the pose mean [x, y, theta] and the pose block P[0:3, 0:3] as they stand AFTER every step -- after its prediction
 * and its last landmark update, motion noise included, NIS-gate rejections honoured: the trajectory with its covariance over
 * time (ATE, pose NEES against ground truth) out of an uploaded stream, which otherwise returns only its last pose.  Off by
 * default.  The log is a device ring of the last `capacity` logged steps, written on every path (per-step kernels, single-launch
 * steps, fused cadences incl. chained and look-ahead runs, the small-state path); switching it on or off changes nothing about
 * the filter (same bits, same scheduling and counters).  A logged STEP is one call of ekf_predict, ekf_update, ekf_step,
 * ekf_step_fetch or ekf_step_detections, or one stream step of ekf_stream_run / ekf_run_stream, whether or not it observes
 * anything.  A step with more than EKF_MMAX landmarks is ONE row (the state after its last pass); a stream step cut by a
 * cadence boundary is one row, written by the cadence that finishes it.  Nothing else writes a row (ekf_add_landmarks,
 * ekf_remove_landmarks, ekf_predict_dense, uploads).  This counter is INDEPENDENT of the innovation log's: a lone ekf_predict
 * is a row here and no step there; both logs may be on together.
 * ekf_log_poses: capacity > 0 allocates the ring (capacity x batch x 12 doubles) and restarts the count at 0; 0 switches the
 * log off and frees it (after a stream synchronisation).
 * ekf_pose_steps: steps logged since the log was switched on.
 * ekf_download_poses: steps [first, first + count) into pose (count x batch x 3) and cov (count x batch x 9, row-major,
 * exactly symmetric; may be NULL).  Blocking and stream-ordered behind everything enqueued; runs no covariance pass or mirror
 * and changes nothing that decides later scheduling.  The last row equals ekf_download_mean's pose bit for bit and a flushed
 * ekf_download_block(0, 0, 3, 3) to rounding.  EKF_ERR_ARG if the range is not inside the last `capacity` logged steps,
 * EKF_ERR_STATE with the log off. */
int ekf_log_poses(ekf_handle *h, int capacity);
int ekf_pose_steps(ekf_handle *h, long long *logged);
int ekf_download_poses(ekf_handle *h, long long first, int count, double *pose, double *cov);

/* NIS validation gate: landmark update j is REJECTED when NIS = y^T S^-1 y > threshold, with the y and S^-1 the filter is about
 * to use -- after the step's prediction and the updates before it, the same NIS the innovation log reports.  A rejected update
 * moves neither mean nor covariance; later updates see the state as if it had never been given.  It still takes its 2 rank
 * slots, so cadence packing and every scheduling counter are the same with the gate on or off.  A NaN NIS is not rejected
 * (EKF_FLAG_NONFINITE as before).  One threshold per handle, on every path that applies landmark updates; off by default, and
 * off means the same bits and launches as without the gate.  For a confidence p the chi-square quantile of 2 degrees of
 * freedom is -2 ln(1 - p) (p = 0.99: 9.21).
 * ekf_set_nis_gate: INFINITY switches the gate off, a finite threshold > 0 on; <= 0 or NaN: EKF_ERR_ARG.  It applies to the
 * launches enqueued after the call, and clears the rejection counters (stream-ordered).
 * ekf_download_gate_counts: updates each trajectory b0 .. b0 + count - 1 rejected since the last ekf_set_nis_gate.  Blocking
 * and stream-ordered, like the other downloads; EKF_ERR_STATE under EKF_FLAG_INTERNAL.
 * ekf_download_innovation_rejections: the innovation log's steps [first, first + count), range rules as
 * ekf_download_innovations, into rejected (count x batch x EKF_AMAX): 1 rejected, 0 applied, -1 beyond a step's m.  The log
 * keeps the true y, S and NIS of a rejected update. */
int ekf_set_nis_gate(ekf_handle *h, double threshold);
int ekf_download_gate_counts(ekf_handle *h, int b0, int count, long long *rejected);
int ekf_download_innovation_rejections(ekf_handle *h, long long first, int count, int *rejected);

/* Per-trajectory noise constants: trajectories [b0, b0+count) use motion_sigma[i] / meas_sigma[i] (the reference's
 * MOTION_MODEL_VARIANCE / MEASUREMENT_MODEL_VARIANCE, src/replay_no_ros.py:15-16, :421, :438) instead of the handle's
 * ekf_config values; a NULL array = the handle's value for that quantity.  Each trajectory's R = diag(s^2, s^2, (s/2)^2) and
 * Q = diag(q^2, q^2) are formed as ekf_create forms the handle's, so one bank can run a grid of noise pairs (a tuning sweep
 * on the innovation log's loglik) on every path that predicts or updates.  Stream-ordered like ekf_set_nis_gate: launches
 * enqueued before the call use the old constants, those enqueued after it the new ones (also between two ekf_stream_run
 * pieces); pose noise already pending keeps the values it was accumulated with.  The call changes neither mean nor
 * covariance nor anything that decides scheduling.  While every trajectory's constants equal the handle's (the default, and
 * again after ekf_set_noise(h, 0, batch, NULL, NULL)) the kernels are the ones without the table: the same bits as a handle
 * that never called it.
 * Not affected: the initial P of ekf_create (from the handle's config), ekf_predict_dense (the caller's Q),
 * landmark_init_var and the association gate.
 * EKF_ERR_ARG (with the handle usable and nothing changed): a range outside the bank, a non-finite value, motion_sigma < 0,
 * meas_sigma <= 0 (Q > 0 keeps S invertible).
 * ekf_get_noise: the values in effect for work enqueued next (a host mirror: does not block); either array may be NULL. */
int ekf_set_noise(ekf_handle *h, int b0, int count, const double *motion_sigma, const double *meas_sigma);
int ekf_get_noise(ekf_handle *h, int b0, int count, double *motion_sigma, double *meas_sigma);

/* State augmentation, src/replay_no_ros.py:341-360: append k landmarks (indices must continue the
 * current count), mean = xy[2*i..], variance = landmark_init_var, zero cross terms. */
int ekf_add_landmarks(ekf_handle *h, int b, int first_index, const double *xy, int k);

/* Landmark removal: marginalise the k landmarks landmarks[0..k) out of trajectory b (b < 0: out of every trajectory, one
 * launch).  Exact for a Gaussian: their rows and columns are deleted, the other landmarks keep their order and every index
 * above a removed one moves down -- mean and covariance equal np.delete, on both axes, of what ekf_download_state returned
 * just before (bit for bit: the pending update is applied first, then stored values only move, on the device, in place).
 * The active bound loses 2 per removed landmark below it.  The device tag table maps a removed tag to -1 (seen again, it
 * is a new landmark appended with landmark_init_var) and renumbers the others; ekf_download_tags drops the removed ones of
 * the last window.  An uploaded stream is refused by ekf_stream_run (EKF_ERR_STATE) until the next ekf_stream_upload.
 * The innovation log, gate counts and noise table are not changed.  Blocking.  k = 0 does nothing; removing every landmark
 * leaves n = 3.  EKF_ERR_ARG (nothing changed): k < 0, an index outside [0, N) of a trajectory concerned, an index twice;
 * EKF_ERR_STATE under EKF_FLAG_INTERNAL or after a call failed half way (as the downloads). */
int ekf_remove_landmarks(ekf_handle *h, int b, const int *landmarks, int k);

/* Direct measurements: tell the filter something in the world frame -- z = x[s] + v, v ~ N(0, R), s a set of state indices.
 * A fix's target is EKF_DIRECT_POSE (x, y, theta from an external localiser, a relocalisation hit, a known start: 3 rows),
 * EKF_DIRECT_POSITION (x, y only: 2 rows) or a landmark index l >= 0 (a surveyed landmark's x, y: 2 rows; anchoring two of them
 * fixes the gauge of the whole map).  Trajectories [b0, b0+count) each bring m[bi] <= stride <= EKF_MMAX fixes: target[bi*stride
 * + j], z (count x stride x 3; the third entry is ignored for 2-row targets) and R (count x stride x 9, row-major 3 x 3: the
 * leading d x d block is the fix's noise covariance, only its upper triangle is read).  All fixes of a trajectory are applied
 * JOINTLY (independent noise: the same posterior as one after the other): their D = sum of d rows are stacked in the order
 * given, R block-diagonal over the fixes,
 *     y = z - mu[s] (the theta row wrapped to [-pi, pi)),  S = P[s,s] + R,  K = P[:,s] S^-1,  mu += K y,  P -= K S K^T
 * on the stored upper triangle; theta of the mean is not re-wrapped (the landmark update does not re-wrap it either).  P is the
 * CURRENT covariance: the pending update is applied first -- a covariance pass the caller pays for, as with ekf_add_landmarks
 * and ekf_remove_landmarks -- then one kernel (k_direct, a workgroup per trajectory: gather of P[s,:], Cholesky of S, the
 * mean, the update's D ranks) and ONE more covariance pass apply the fixes of the whole call.
 * nis[bi] = y^T S^-1 y and dof[bi] = D (either may be NULL; 0 and 0 for m[bi] = 0).  gate (count doubles; NULL or INFINITY:
 * none): a trajectory whose NIS exceeds gate[bi] is REJECTED AS A WHOLE, its mean and covariance stay bit for bit (the chi-square
 * quantile of D degrees of freedom is the natural threshold; the handle's NIS gate is one of 2 degrees and does not apply
 * here).  A trajectory whose S fails to factor (a pivot <= 0 or not finite) is rejected the same way, on the device, and gets
 * EKF_FLAG_NONFINITE.  applied[bi] (may be NULL): 1 applied, 0 rejected or m[bi] = 0.  A trajectory with m[bi] = 0, or outside
 * the range, is untouched bit for bit (the pass adds exact zeros to it).
 * Blocking, and stream-ordered behind everything enqueued.  Writes no innovation-log or pose-log row (like ekf_add_landmarks
 * and ekf_remove_landmarks), changes no gate counter, noise row, size, tag table or uploaded stream (which stays runnable) and
 * leaves the active bound as it is: a direct update changes P(a, b) only where both a and b are correlated with s, it creates no
 * correlation (a fix on a never-observed landmark touches its own 2 x 2 block and mean only).  Afterwards nothing is pending:
 * a following ekf_stream_run forms fused cadences as after any flush; a handle on the small-state path stays on it.
 * EKF_ERR_ARG (nothing changed, the handle usable): a bad trajectory range, stride outside 1..EKF_MMAX, m[bi] outside
 * 0..stride, a landmark index outside that trajectory's map, the same target twice in one trajectory, EKF_DIRECT_POSE and
 * EKF_DIRECT_POSITION (or one of them twice) in one trajectory, a non-finite z, R or gate, gate[bi] <= 0, an R block that is
 * not positive definite (leading minors of the d x d block), NULL target, z, R or m.  EKF_ERR_STATE if a trajectory of the
 * range carries EKF_FLAG_INTERNAL or an earlier call failed half way (as the downloads).
 * Not measured yet (tools/direct_update_time.py writes profiles/direct_update.txt). */
#define EKF_DIRECT_POSE (-1)     /* target: x, y, theta (3 rows) */
#define EKF_DIRECT_POSITION (-2) /* target: x, y        (2 rows) */
                                 /* target l >= 0: landmark l's x, y (2 rows) */
int ekf_update_direct(ekf_handle *h, int b0, int count, const int *target, const double *z, const double *R,
                      const int *m, int stride, const double *gate, double *nis, int *dof, int *applied);

/* Linear measurement update: any measurement the caller can write as  r = H_s x[s] + v,  v ~ N(0, R),  over a small SUB-STATE
 * -- "landmark j lies 0.585 m east of landmark i", "these two landmarks are the same tag" (l_i - l_j = 0, then
 * ekf_remove_landmarks), a range-only beacon, a bearing-only camera, a lane-relative heading, any model linearised at the
 * current mean.  The sub-state is named exactly as ekf_download_joint names it: trajectory bi of [b0, b0+count) lists k[bi] <=
 * lstride <= EKF_LINEAR_LMAX landmarks in landmarks[bi*lstride + 0..k[bi]), in any order and none twice; its sub-state is
 * [x, y, theta, l_j0 x, l_j0 y, l_j1 x, ...] in the order given, ns = 3 + 2*lstride; k[bi] = 0 is the pose alone.
 * H is count x dstride x ns (row-major), r count x dstride, R count x dstride x dstride (a dense noise covariance of which only
 * the upper triangle is read).  Trajectory bi uses the leading d[bi] <= dstride <= EKF_LINEAR_ROWS rows and the leading
 * 3 + 2*k[bi] columns of H; nothing beyond those is read.
 * innovation == 0: r is the measurement z and the device forms y = z - H_s mu[s] from the mean it is about to update; no row is
 * wrapped (a linear constraint that involves theta has to come as an innovation).  innovation == 1: r is the innovation y
 * itself -- the form for a model linearised by the caller at the mean ekf_download_joint returned (both calls are blocking and
 * nothing moves between them).  Jointly over all rows,
 *     S = H_s P[s,s] H_s^T + R,   mu += P[:,s] H_s^T S^-1 y,   P -= P[:,s] H_s^T S^-1 H_s P[s,:]
 * on the stored upper triangle; theta of the mean is not re-wrapped.
 * What follows is ekf_update_direct's, word for word where it applies (see there): P is the CURRENT covariance, the pending
 * update is applied first -- a covariance pass the caller pays for --, then one kernel (k_linear, a workgroup per trajectory)
 * and ONE more covariance pass for the whole call.  nis[bi] = y^T S^-1 y (may be NULL; 0 for d[bi] = 0).  gate (count doubles;
 * NULL or INFINITY: none): a trajectory whose NIS exceeds gate[bi] is REJECTED AS A WHOLE, its mean and covariance stay bit for
 * bit.  A trajectory whose S fails to factor (a pivot <= 0 or not finite) is rejected the same way, on the device, and gets
 * EKF_FLAG_NONFINITE.  applied[bi] (may be NULL): 1 applied, 0 rejected or d[bi] = 0.  A trajectory with d[bi] = 0, or outside
 * the range, is untouched bit for bit.  Blocking, and stream-ordered behind everything enqueued.  Writes no innovation-log or
 * pose-log row, changes no gate counter, noise row, size, tag table or uploaded stream (which stays runnable).  Afterwards
 * nothing is pending; a handle on the small-state path stays on it.
 * THE ACTIVE BOUND is where the call differs: a general row ties its targets together, so for every trajectory of the range
 * with d[bi] > 0 the bound is raised to cover the highest landmark of its sub-state before the kernel runs, as a landmark
 * update of that landmark raises it (also where the gate then rejects: the bound is conservative).  There is no closed-form
 * branch for never-observed landmarks.  (The cross terms of P_base beyond the old bound are exact zeros: ekf_upload_state_diag
 * and ekf_add_landmarks write them, ekf_remove_landmarks moves them unchanged, and nothing writes beyond the bound; the
 * stream's own rise of the bound relies on the same.)
 * A zero row of H is legal (S keeps R's row).
 * EKF_ERR_ARG (nothing changed, the handle usable): a bad trajectory range, lstride outside 1..EKF_LINEAR_LMAX, dstride outside
 * 1..EKF_LINEAR_ROWS, k[bi] outside 0..lstride, d[bi] outside 0..dstride, a landmark index outside that trajectory's map or
 * named twice, a non-finite H, r, R or gate, gate[bi] <= 0, an R whose leading d x d block is not positive definite (Cholesky
 * of its upper triangle), NULL landmarks, k, H, r, R or d.  EKF_ERR_STATE if a trajectory of the range carries
 * EKF_FLAG_INTERNAL or an earlier call failed half way (as the downloads).
 * Measured on one MI355X (tools/linear_update_time.py, profiles/linear_update.txt), per call for the whole bank: 32 x N = 2000
 * 1.3 ms with 4 rows per trajectory, 1.9 ms with 32 (k_linear 0.04 / 0.44 ms, the pass 0.68 ms; ekf_update_direct with as many rows
 * 1.3 / 2.0 ms); 1 x N = 2000 with 32 rows 0.5 ms, of which k_linear's one workgroup is 0.39 ms. */
int ekf_update_linear(ekf_handle *h, int b0, int count, const int *landmarks, const int *k, int lstride,
                      const double *H, const double *r, const double *R, const int *d, int dstride,
                      int innovation, const double *gate, double *nis, int *applied);

/* Fork / checkpoint on the device: copy the complete filter state of trajectory src_b[i] of `src` to trajectory dst_b[i] of
 * `dst`, i < k, without leaving HBM.  src == dst is allowed (fork inside a bank); otherwise both handles must be on the same
 * device.  One source may fan out to many destinations (one launch for all pairs; a source tile is read once for up to 32 of
 * its destinations).  Afterwards ekf_download_state(dst, d) equals ekf_download_state(src, s) bit for bit, mean and
 * covariance, and ekf_state_size is equal; the active bound, the device tag table's row and the last window's tags
 * (ekf_download_tags, ekf_download_tag_index) and the sticky flags EKF_FLAG_NONFINITE / EKF_FLAG_ASSOC are the source's --
 * they describe that state's history -- so that the same calls on both from there on give the same bits.
 * NOT copied, being properties of the slot and not of the state: the slot's noise row (ekf_set_noise), gate counters,
 * innovation-log and pose-log rows (the call writes no log row, like ekf_remove_landmarks), the inputs of an uploaded stream.
 * The uploaded stream of `dst` stays usable exactly as after ekf_upload_state: ekf_stream_run checks that the state has the
 * landmarks it observes.
 * The pending update of BOTH handles is applied first (as by every call that rewrites a covariance: a pass the caller pays
 * for, like ekf_upload_state, and ekf_debug_cadences / ekf_profile_passes and what is pending afterwards change accordingly);
 * stored values then only move.  The handles may differ in n_max and hence in device layout (row stride, column panels);
 * the source's n must fit the destination's n_max.  Blocking, and stream-ordered behind everything enqueued on both handles.
 * k = 0 does nothing.  EKF_ERR_ARG (nothing changed, both handles usable; the message is `dst`'s ekf_last_error): k < 0, a
 * NULL array with k > 0, an index outside its bank, a destination named twice, with src == dst a trajectory that is both a
 * source and a destination (s == d included), handles on different devices, a source n above the destination's n_max.
 * EKF_ERR_STATE: a source carries EKF_FLAG_INTERNAL or an earlier call on `src` failed half way.  A DESTINATION in that
 * condition is cleared by the copy, as by an upload: a spare slot or handle is a recovery path.
 * Measured (profiles/copy_trajectories.txt): a 1 -> 31 fork at 32 x N = 2000 (2.05 GB moved) takes 0.43 ms, 0.77 of the
 * measured 6.29 TB/s copy rate of the part, against 62 ms through ekf_download_state + 31 x ekf_upload_state. */
int ekf_copy_trajectories(ekf_handle *dst, const int *dst_b, ekf_handle *src, const int *src_b, int k);

/* Map joining on the device: append the map of trajectory src_b[i] of `src` to trajectory dst_b[i] of `dst`, i < k, in one launch
 * (k_join) -- sequential map joining (map locally in a small filter, join the local map into the global one every so often) and
 * the merge of two maps related by a rigid transform.  For a pair (A = [r_A; L_A] of n_A = 3 + 2 N_A, B = [r_B; L_B]) a base
 * frame g = (t, phi) with covariance Sigma and cross terms G (3 x n_A, the covariance of g with A's state) maps every item of B
 * into A's frame; with R = rot(phi), J2 = [[0, -1], [1, 0]], Jacobians at the current means:
 *   landmark  l' = t + R l                      A_l = [I2 | J2 R l]                  B_l = R
 *   pose      p' = (t + R p_xy, phi + theta_B)  A_p = [[I2, J2 R p_xy], [0 0 1]]     B_p = diag(R, 1)   (theta is not re-wrapped)
 *   P'[c1, c2] = A_c1 Sigma A_c2^T + B_c1 P_B[c1, c2] B_c2^T      P'[a, c] = G[:, a]^T A_c^T      P'[L_A, L_A], L_A: unchanged
 * T == NULL (sequential): the source's frame IS the destination's current pose -- g = r_A, Sigma = P_A[r, r], G = P_A[r, :] --
 * and the destination's pose is REPLACED by r_A (+) r_B (rows 0..2 become A_p G over L_A).  N_B = 0 moves the pose alone.
 * T != NULL (explicit): g = T[i] = (x, y, phi) with covariance covT[i] (3 x 3 row-major, the upper triangle is read, may be all
 * zero), independent of both maps (G = 0): the destination's pose, its rows and every entry of A stay bit for bit, the source's
 * pose is dropped, the cross terms between A and the appended part are exact zeros.
 * Either way the source's N_B landmarks are appended at landmark indices N_A .. N_A + N_B - 1 in the source's order; first[i]
 * (may be NULL) receives N_A.  The destination's size becomes n_A + 2 N_B, its active bound the new size; existing indices do not
 * move, so its uploaded stream stays runnable; no log row is written and no gate counter, noise row or sticky flag changes; the
 * last window's tags (ekf_download_tags) stay.  The source is not written.  A handle on the small-state path stays on it.
 * Device tag table: an appended landmark keeps its source tag at its new index, unless the destination's map already holds that
 * tag -- then the destination's entry stays, the appended landmark is untagged, and twin[i * twin_stride + j] (may be NULL) is
 * the destination landmark that carries the tag of source landmark j; -1 otherwise, and throughout where either side has no
 * table.  Fusing twins is the caller's: constrain them (ekf_update_linear) and remove one (ekf_remove_landmarks); INTEGRATION.md.
 * src == dst is allowed; otherwise both handles must be on the same device; a source may be named several times.  What is pending
 * on BOTH handles is applied first (a pass the caller pays for).  Blocking, and stream-ordered behind everything enqueued on
 * both handles.  k = 0 does nothing.  Every entry is a fixed sequence of at most 13 products: the same pair gives the same bits
 * whatever else the launch carries.  With ekf_set_option("profile_kernels", 1) the launch is class 6 of ekf_profile_read_class.
 * EKF_ERR_ARG (nothing changed, both handles usable; the message is `dst`'s ekf_last_error): k < 0, a NULL index array with
 * k > 0, an index outside its bank, a destination named twice, with src == dst a trajectory that is both a source and a
 * destination, handles on different devices, n_A + 2 N_B above the destination's n_max, exactly one of T / covT given, a
 * non-finite T or covT, a negative diagonal of covT or c_ij^2 > c_ii c_jj, `twin` given with twin_stride below the largest N_B.
 * EKF_ERR_STATE: a source OR a destination carries EKF_FLAG_INTERNAL or an earlier call on its handle failed half way (a
 * destination is read here, not only overwritten).
 * Measured: profiles/join.txt. */
int ekf_join_maps(ekf_handle *dst, const int *dst_b, ekf_handle *src, const int *src_b, int k,
                  const double *T /* k x 3 or NULL */, const double *covT /* k x 9 or NULL */,
                  int *first /* k, may be NULL */, int *twin /* k x twin_stride, may be NULL */, int twin_stride);

/* Change of frame on the device: move trajectories [b0, b0+count) of a running filter into another frame, in place, in one launch
 * (k_transform) -- the world frame became known after the filter had started at the origin (a surveyed tag map, a Vicon
 * alignment): align first, then anchor (ekf_update_direct), whatever the offset.  T[3*bi..] = (x, y, phi) is the OLD frame
 * expressed in the NEW one, ekf_join_maps' explicit-mode convention; cov[9*bi..] its covariance (3 x 3 row-major, the upper
 * triangle is read), or cov == NULL: the frame is known exactly.  With R = rot(phi), J2 = [[0, -1], [1, 0]], Jacobians at the
 * current means, for every item of the filter's own state:
 *   landmark  l' = t + R l                      A_l = [I2 | J2 R l]                  B_l = R
 *   pose      p' = (t + R p_xy, theta + phi)    A_p = [[I2, J2 R p_xy], [0 0 1]]     B_p = diag(R, 1)   (theta is not re-wrapped)
 *   P'[c1, c2] = B_c1 P[c1, c2] B_c2^T + A_c1 Sigma A_c2^T        (the second term only where cov is given)
 * -- exact for a Gaussian state: no rank, no covariance pass, one read and one write of the stored upper triangle (of a diagonal
 * block: three entries; a download afterwards is exactly symmetric).  What is pending is applied first (a pass the caller pays
 * for); afterwards nothing is pending.  Blocking, and stream-ordered behind everything enqueued.  count = 0 does nothing.
 * T = (0, 0, 0) with cov == NULL leaves a trajectory bit for bit.  cov == NULL otherwise: the active bound stays, and what is an
 * exact zero because of it stays +0.0.  cov given: every item becomes correlated with every other, the active bound becomes the
 * size (as after ekf_join_maps).  Unchanged: sizes, the tag table, noise rows, gate counters, sticky flags, innovation-log and
 * pose-log rows (the call writes no log row, like ekf_remove_landmarks and ekf_join_maps); the uploaded stream stays runnable
 * (ranges, bearings and increments are frame-free); trajectories outside the range stay bit for bit.  The world positions of the
 * last window's tags (ekf_download_tags: xw, yw) are mapped through T, err stays.  A factor held by ekf_factor is a snapshot of
 * the state it was taken from, as after any other change of state.  A handle on the small-state path stays on it.  Every entry is
 * a fixed sequence of at most 13 products: the same trajectory gives the same bits alone or in a bank.  With
 * ekf_set_option("profile_kernels", 1) the launch is class 8 of ekf_profile_read_class.
 * EKF_ERR_ARG (nothing changed, the handle usable): count < 0, a range outside the bank, T == NULL with count > 0, a non-finite T,
 * a non-finite cov, a negative diagonal entry of cov, c_ij^2 > c_ii c_jj, or a negative determinant of its symmetrised upper
 * triangle (beyond the rounding of the determinant itself).  EKF_ERR_STATE: a trajectory of the range carries EKF_FLAG_INTERNAL or
 * an earlier call on the handle failed half way.
 * Measured on one MI355X (tools/transform_time.py, profiles/transform.txt), call + sync / kernel alone, with or without cov:
 * 32 x N = 2000 1.25 / 1.22 ms (0.70 of ekf_copy_trajectories' rate for the same bytes), 1 x N = 2000 75 / 39 us, 1 x N = 8000
 * 0.69 / 0.65 ms, 256 x N = 20 (small-state path) 70 / 10 us. */
int ekf_transform(ekf_handle *h, int b0, int count, const double *T /* count x 3 */, const double *cov /* count x 9 or NULL */);

/* Pinned (page-locked, device-visible) host memory for the arrays a binding hands to its caller.  The reference's loop
 * gets a fresh n x n covariance back from every call (src/replay_no_ros.py:229-237, :482): in freshly allocated pageable
 * memory a 128 MB download first faults in and pins 32 768 pages (5 ms on top of 2.3 ms of PCIe time at N = 2000); the
 * Python binding recycles buffers from these instead.  ekf_host_alloc returns NULL when the allocation fails. */
void *ekf_host_alloc(size_t bytes);
void ekf_host_free(void *p);

/* predict(): src/replay_no_ros.py:368-430 for every trajectory (lin[b], ang[b]).  O(n) work. */
int ekf_predict(ekf_handle *h, const double *lin, const double *ang);

/* Prediction with a motion model of the caller's: wheel odometry that arrives as a pose increment with its own 3 x 3 covariance,
 * visual odometry, an IMU heading, another kinematic model, slip noise that grows with curvature -- anything the caller can
 * linearise at the current pose.  Trajectory bi of [b0, b0+count) brings the NEW pose mean pose[3*bi..] = [x, y, theta], taken
 * verbatim (the caller wraps theta), F[9*bi..] = d(new pose)/d(old pose) (row-major 3 x 3) and the process noise Q[9*bi..]
 * (row-major 3 x 3, the upper triangle is read, positive SEMI-definite).  For every applied trajectory (apply == NULL: all;
 * apply[bi] == 0 leaves that trajectory bit for bit), with G = blockdiag(F, I):
 *     mu[0:3] = pose,   P[r,r] <- F P[r,r] F^T + Q,   P[r,j] <- F P[r,j]  (j >= 3)
 * on the stored upper triangle: rows 0..2 and nothing else.  P is the CURRENT covariance -- P_base + the pending ranks + the
 * pending pose noise -- and, like the built-in prediction, the call costs no rank and NEVER a covariance pass, also while ranks
 * are pending: one kernel (k_predict_pose) gathers the current x = P(0..2, j) as the read-only queries do, with their bounds, and
 * adds (F - I) x to P_base in place (the pose block: (F P_rr F^T + Q) - P_rr, P_rr the current block); the pending V / W and
 * pose noise are not written and the pass applies them as ever.  Where nothing is pending F x is written directly, no
 * difference of nearly equal numbers.  In both forms F = I, Q = 0 leaves the covariance bit for bit.  O(n) per trajectory,
 * O(n kb) with kb ranks pending; every sum runs in a fixed order: a trajectory's result does not depend on its slot or on its
 * neighbours.
 * Left alone: landmark means and every P(a, b) with a, b >= 3, bit for bit; sizes, tag table, noise rows, gate counters, sticky
 * flags, the uploaded stream (which stays runnable) and the active bound (F mixes the pose rows among themselves only; beyond the
 * bound they are exact zeros and stay so); ekf_profile_passes and ekf_debug_cadences / _chained / _lookaheads; what is pending
 * -- the call is never counted for "flush_every" or "rank_limit"; a handle on the small-state path stays on it.
 * ASYNCHRONOUS, enqueued like ekf_predict: stream-ordered behind everything enqueued (also what a chained run left on the
 * handle's second stream), the records go up as a step's do, and the host arrays are borrowed for the call only.  It blocks
 * only where ekf_predict does (the input ring coming round, sizes a device-side association grew).  Pose log: the call is a
 * logged step, one row, as a lone ekf_predict; innovation log: no step.
 * With ekf_set_option("profile_kernels", 1) the launch is class 7 of ekf_profile_read_class.
 * EKF_ERR_ARG (nothing changed, the handle usable): a bad trajectory range, NULL pose, F or Q, and for an applied trajectory a
 * non-finite entry of pose, F or Q, a Q with a negative diagonal entry, with q_ij^2 > q_ii q_jj, or with a negative determinant
 * of its symmetrised upper triangle (beyond the rounding of the determinant itself: a Q of rank 1 or 2 is legal).  An all-zero Q
 * and a singular F are legal.  EKF_ERR_STATE after an earlier call failed half way.  Like ekf_predict the call does not read the
 * sticky flags back (that would synchronise): a trajectory under EKF_FLAG_INTERNAL is reported by the next blocking call, as
 * ever.
 * Measured on one MI355X (tools/predict_linear_time.py, profiles/predict_linear.txt), call + sync for the whole bank beside
 * ekf_predict at the same state: 32 x N = 2000 28 against 26 us with nothing pending (k_predict_pose 7 us), 43 against 47 us with
 * 78 ranks pending (k_predict_pose 21 us); 1 x N = 2000 27 against 24 us and, with 78 ranks pending, 37 against 28 us (a
 * latency-bound gather: 16 us); 1 x N = 8000 under an active bound of 83 27 against 24 us; 256 x N = 20 30 against 26 us.  The
 * routes it replaces: the host round trip 0.68 s for the bank of 32, ekf_predict_dense 8.8 ms per N = 2000 trajectory. */
int ekf_predict_linear(ekf_handle *h, int b0, int count,
                       const double *pose /* count x 3 */, const double *F /* count x 9 */, const double *Q /* count x 9 */,
                       const int *apply /* count, may be NULL */);

/* update(): src/replay_no_ros.py:436-480, sequential over idx[b*stride + 0..m[b]) in that order. */
int ekf_update(ekf_handle *h, const int *idx, const double *range, const double *bearing,
               const int *m, int stride);

/* step() = predict + update fused into one pass over P (what EKF_pose_estimation does after
 * association/augmentation, src/replay_no_ros.py:363-482).  Asynchronous on the handle's stream. */
int ekf_step(ekf_handle *h, const double *lin, const double *ang, const int *idx,
             const double *range, const double *bearing, const int *m, int stride);

/* Localisation on a FROZEN MAP: pose-only steps for a run that drives on a map it considers finished -- the second lap, a fleet of
 * forked hypotheses relocalising against one map, the localisation phase behind a noise tuning.  The Schmidt-Kalman ("consider")
 * update: per observation of landmark l (state indices t = 3 + 2l, t + 1), H = [H_p | H_l] from the filter's own linearisation at
 * the current pose and the frozen landmark mean, S = H P H^T + R on the five indices exactly as ekf_step forms it, and the gain
 * K = [K_p; 0] with K_p = (P H^T)[0:3] S^-1: the landmarks' uncertainty and their correlations with the pose enter S and the pose
 * rows, the landmarks themselves do not move.  pose += K_p y, and with the Joseph form (I - K H) P (I - K H)^T + K R K^T
 *     P[r,r] <- P[r,r] - K_p S K_p^T,   P[r,c] <- (I - K_p H_p) P[r,c] - K_p H_l P[t:t+2, c]  (c >= 3),   P[a,b] as it was (a, b >= 3)
 * Unlike "treat the map as perfect" the result stays consistent; it differs from full SLAM's except on an exactly known map
 * (P[a,b] = 0 for all b where a >= 3: there the two agree to rounding).  No claim is made that the pose covariance exceeds full
 * SLAM's: with sequentially re-linearised updates it need not.
 * ekf_localize_step: prediction (ekf_predict's motion model and noise) + the frozen-map update of idx[b*stride + 0..m[b]) in that
 * order, for the whole bank; ekf_localize_update: the update alone, behind ekf_predict, ekf_predict_linear or an odometry
 * prediction; ekf_localize_run: steps [first, first + count) of the uploaded stream (ekf_stream_upload) in localisation mode, back
 * to back without a host synchronisation -- the same two kernels per step reading the stream's records, the same bits as the same
 * steps through ekf_localize_step.  Arguments as ekf_step's / ekf_stream_run's; more than EKF_MMAX observations of a trajectory
 * run as several passes, the prediction in the first.  One difference: an index MAY come twice in one call (the second observation
 * is linearised at the pose the first one left; the SLAM update keys observations by index and refuses that).
 * Two launches per step (pass): k_loc_solve, one wave per trajectory, runs the prediction and the sequential chain on the
 * compressed set {0, 1, 2, t_j, t_j + 1} and collapses the step to x_c <- A x_c + sum_j B_j P[t_j:t_j+2, c]; k_loc_rows applies
 * that to every column of the pose rows in one fully parallel O(n m) launch.  Never a covariance pass, no rank.
 * Written: rows 0..2 of the stored triangle below the (raised) active bound, the pose mean, the sticky flags.
 * Left alone, bit for bit: landmark means and every P(a, b) with a, b >= 3; sizes, tag table, noise rows, the uploaded stream
 * (which stays runnable); ekf_profile_passes and ekf_debug_cadences / _chained / _lookaheads do not move, and the call is never
 * counted for "flush_every" or "rank_limit"; a handle on the small-state path stays on it (the kernels work on P_base in global
 * memory in both layouts, and read their records from the pinned ring as that path's steps do).
 * Ranks pending at entry: the call first runs the ordinary covariance pass, once (as ekf_flush), and then works on P_base with
 * nothing pending; it leaves nothing pending, so later localisation calls run no pass at all.
 * Active bound: an observation correlates the pose with the landmark it names: the call raises the bound over the highest
 * landmark observed, as ekf_update_linear does (also over one the NIS gate then rejects).
 * On this path too: ekf_set_noise's row supplies R and the motion noise; the NIS gate rejects an observation with K_p = 0 -- the
 * state is then BIT-IDENTICAL to the same call without that observation (given the same active bound), the gate counter counts
 * it and the other observations of the step are applied; the innovation log gets one step per call (y, S, NIS, the rejected bit),
 * the pose log one row per call (a lone ekf_localize_update logs as a lone ekf_update); the config flags
 * enable_measurement_model, enable_circular_interpolation, disable_motion_model and arc_threshold act as on the other paths.
 * Degenerate geometry (pose on the landmark, q = 0) gives NaN as there and EKF_FLAG_NONFINITE.
 * Every sum runs in observation order: a trajectory's bits depend neither on its slot nor on its neighbours.
 * ASYNCHRONOUS like ekf_step.  EKF_ERR_ARG (nothing changed): NULL arrays, a count outside [0, stride], an index outside the
 * trajectory's map; ekf_localize_run: EKF_ERR_STATE for a range outside the uploaded stream or a stream the state no longer
 * fits, as ekf_stream_run.  EKF_ERR_STATE after an earlier call failed half way.  The sticky flags are not read back.
 * With ekf_set_option("profile_kernels", 1) the launches are classes 9 (k_loc_solve) and 10 (k_loc_rows) of ekf_profile_read_class.
 * Measured on one MI355X (tools/localize_time.py, profiles/localize.txt), device time per step for the whole bank, m = 8, every
 * state index active, 40 steps behind a dense start; the passes ekf_step causes are charged to it: 32 x N = 2000 30 us
 * (ekf_localize_run 27) against ekf_step 186 and ekf_stream_run 160; 1 x N = 8000 23 (20) against 93 and 78; 1 x N = 2000 22 (19)
 * against 31 and 17 -- NOT faster than the chained SLAM cadence there: two launches and a sequential chain of ~1.5 us per
 * observation in one wave are the floor (k_loc_solve 14 us, k_loc_rows 8 us between their event pairs) --; 256 x N = 20 24 (19)
 * against 19 and 10: slower than the small-state path, which keeps P in LDS across a whole stream.  The map staying fixed is
 * the feature either way. */
int ekf_localize_step(ekf_handle *h, const double *lin, const double *ang, const int *idx,
                      const double *range, const double *bearing, const int *m, int stride);
int ekf_localize_update(ekf_handle *h, const int *idx, const double *range, const double *bearing,
                        const int *m, int stride);
int ekf_localize_run(ekf_handle *h, int first, int count);

/* ekf_step followed by ekf_download_state(h, b, mu, P, n), as ONE call: one iteration of the reference's loop
 * (`mean, covariance, tags = EKF_pose_estimation(...)`, src/replay_no_ros.py:229-237; the return at :482 hands back the
 * whole state every call).  Same results as the two calls.  On the small-state path (option "small_state") the step's
 * own launch writes trajectory b's mean, mirrored covariance and flags into pinned host memory: one kernel launch and one
 * synchronisation per call; otherwise the two calls are made for the caller.  Blocking; n must equal the state size. */
int ekf_step_fetch(ekf_handle *h, const double *lin, const double *ang, const int *idx, const double *range,
                   const double *bearing, const int *m, int stride, int b, double *mu, double *P, int n);

/* Device-side front end (association, 1.5 m gate, per-tag averaging, augmentation: src/replay_no_ros.py:280-360)
 * followed by the fused step: one window of raw AprilTag detections per trajectory, frames concatenated in
 * order -- count[b] detections at tag_id / pose_t (x, y, z of tag.pose_t) / pose_err [b*stride + i].  The tag-id
 * -> landmark-index table lives on the device (ekf_download_tag_index); ekf_download_tags returns what the
 * reference returns as tags_positions for the last window.  ekf_set_association sets gate and IGNORE_TAGS.
 * EKF_ERR_ARG (a NULL array it needs, stride < 0, a count outside [0, min(stride, EKF_DMAX)]) changes nothing: the window is
 * checked before anything is allocated, pushed or taken from the input ring. */
int ekf_set_association(ekf_handle *h, double gate_range, const int *ignore_tags, int n_ignore);
int ekf_step_detections(ekf_handle *h, const double *lin, const double *ang, const int *count, const int *tag_id,
                        const double *pose_t, const double *pose_err, int stride);
int ekf_download_tags(ekf_handle *h, int b, int *m, int *idx, int *tag_id, double *xw, double *yw, double *err,
                      double *range, double *bearing);     /* arrays of EKF_AMAX entries */
int ekf_download_tag_index(ekf_handle *h, int b, int *tag_of_index, int capacity, int *n_landmarks);
int ekf_upload_tag_index(ekf_handle *h, int b, const int *tag_of_index, int n_landmarks);

/* Localisation from raw detections: the device-side front end in front of ekf_localize_step, for a lap over a finished map.
 * Arguments and argument checks are ekf_step_detections'; the semantics are ekf_localize_step's on whatever the window MATCHES.
 * k_loc_associate, one wave per trajectory, walks the window exactly as the mapping front end does -- chunks of 64 detections,
 * IGNORE_TAGS, the gate of ekf_set_association, ids outside [0, 1024) set EKF_FLAG_ASSOC, one slot per distinct tag in order of
 * first appearance, per-tag averaging, range and bearing, the world guess from the pose before the prediction: a tag's averaged
 * (range, bearing) has the bits ekf_step_detections would give it -- with one difference: the map is frozen.  A tag the table
 * does not know, or whose table entry points at or beyond the trajectory's landmark count, is UNMATCHED: it is skipped without
 * a flag and its id is kept for ekf_download_unmatched.  More than EKF_AMAX distinct matched tags: the surplus is dropped with
 * EKF_FLAG_ASSOC.  The matched tags then run as ekf_localize_step runs them -- k_loc_solve and k_loc_rows, a second pair for the
 * tags beyond EKF_MMAX -- with no host round trip in between: the state ends BIT FOR BIT as after ekf_localize_step with the idx,
 * range and bearing ekf_download_tags reports, and the innovation log and the pose log get the same rows.
 * Never written: the tag table (ekf_download_tag_index returns what it returned before), the sizes, the landmark means, every
 * P(a, b) with a, b >= 3.  Ranks pending at entry are applied first, once.  The active bound is raised over the matched landmarks
 * on the device.  ekf_set_noise's rows, the NIS gate, enable_measurement_model (off: prediction only) and the "active_bound"
 * option act as on ekf_localize_step.  ASYNCHRONOUS like ekf_step_detections; EKF_ERR_ARG changes nothing; a failure behind the
 * first launch leaves every trajectory undefined (EKF_ERR_STATE until uploaded again), as for ekf_localize_step.
 * ekf_download_tags returns the matched tags of the window (n landmarks or fewer, update order).
 * ekf_download_unmatched: the distinct unmatched ids of trajectory b's last localisation window in order of first appearance --
 * *m their number, the first min(*m, capacity, EKF_AMAX) of them in tag_id (may be NULL with capacity 0).  Blocking.
 * EKF_ERR_STATE if no localisation window has run on the handle.
 * Measured on one MI355X (tools/localize_detections_time.py, profiles/localize_detections.txt), 8 tags x 3 frames per trajectory:
 * k_loc_associate alone 14 - 16 us whatever the bank (class 11 of ekf_profile_read_class).  Through the Python binding a window
 * costs 679 us for 32 x N = 2000, 45 us for 1 x N = 2000 and 5.3 ms for 256 x N = 20 -- host-bound, as ekf_step_detections is on
 * the same window (737, 48, 5.3 ms): the binding packs one detection at a time -- against 6.5 ms, 254 us and 29.6 ms for tag
 * table + mean download, host association and ekf_localize_step. */
int ekf_localize_detections(ekf_handle *h, const double *lin, const double *ang, const int *count,
                            const int *tag_id, const double *pose_t, const double *pose_err, int stride);
int ekf_download_unmatched(ekf_handle *h, int b, int *m, int *tag_id, int capacity);

/* A bank of pose hypotheses on ONE frozen map: global localisation (the kidnapped robot) with hundreds or thousands of candidate
 * poses.  A forked slot of a handle carries its own copy of the whole stored triangle, 8 n^2 bytes; on a frozen map every copy
 * is identical, and what differs between two hypotheses is the pose mean, the pose block and the pose rows P(0..2, :).  The bank
 * stores the map once and 24 bytes per column of the handle's row stride + 1040 bytes per hypothesis.  Measured on one MI355X
 * (tools/hypotheses_time.py, profiles/hypotheses.txt; m = 8, shared observations, call + sync per step for all hypotheses):
 * N = 2000: K = 32 31 us (ekf_localize_step on 32 forked slots: 30 us) in 135 MB against 4.2 GB, K = 1024 162 us, K = 4096 729 us;
 * N = 8000, K = 32: 35 us against 37 us, 2.1 GB against 68 GB.  ekf_hyp_adopt: 81 us at N = 2000, 421 us at N = 8000.
 * ekf_hyp_create applies what is pending on `h`, copies slot b's stored triangle, mean and tag-table row -- a SNAPSHOT: nothing
 * the handle does afterwards reaches the bank, and nothing needs invalidating -- and seeds `count` hypotheses (1 .. 65536) with the
 * slot's pose, pose block and pose rows.  The bank takes the handle's config flags, the slot's noise pair (ekf_set_noise), the
 * handle's NIS gate threshold and, at creation, the slot's active bound.  Blocking.  Errors go to ekf_last_error of `h`.
 * ekf_hyp_step / ekf_hyp_update are ekf_localize_step / ekf_localize_update for every hypothesis: the same kernel arithmetic in the
 * same order, so a hypothesis ends BIT FOR BIT as a forked slot given the same calls would, whatever `count` and wherever it sits
 * in the bank.  motion_stride 0: lin[0], ang[0] for every hypothesis, 1: lin[k], ang[k].  obs_stride 0: ONE list of m[0]
 * observations idx / range / bearing [0, m[0]) for every hypothesis (tags carry their ids: the common case; one record is
 * uploaded), 1: hypothesis k's m[k] observations at [k * stride, k * stride + m[k]).  m <= EKF_MMAX per call: a longer list is
 * refused; split it into a step and update-only calls.  An index may come twice; indices are checked against the map.
 * Every observation, whether or not the gate then rejects it, adds -1/2 (y^T S^-1 y + ln det S + 2 ln 2 pi) to the hypothesis's
 * loglik (a term that is not finite is left out) and counts in n_obs; a rejection counts in n_rej and leaves pose, block and rows
 * bit-identical to the call without that observation.  ASYNCHRONOUS on the bank's own stream.
 * ekf_hyp_reset: the kidnapped-robot entry for hypotheses [k0, k0 + count): pose mean and pose block (cov: 3 x 3 row-major, the
 * upper triangle is read) set, the pose rows zeroed, loglik, counters and flags cleared, the bound back to the map's -- what
 * ekf_predict_linear with F = 0, Q = cov does to a slot.  Asynchronous.
 * ekf_hyp_download (blocking; every output may be NULL): pose count x 3, cov count x 9 (the block, mirrored), loglik, n_obs, n_rej
 * and the sticky flags (EKF_FLAG_NONFINITE) of hypotheses [k0, k0 + count).  ekf_hyp_download_rows: hypothesis k's P(0..2, 0..n) as
 * 3 x n row-major, n the map's size.
 * ekf_hyp_set_nis_gate: as ekf_set_nis_gate, for the bank (the rejections are the hypotheses' n_rej).
 * ekf_hyp_adopt writes hypothesis k's pose mean, pose block and pose rows into slot b of `h` -- any handle on the same device
 * whose slot b has the map as its frozen part.  Blocking: it waits for the bank's stream, applies what is pending on `h`, and
 * compares on the device the slot's size, landmark means and every stored P(a, c), 3 <= a <= c < n, with the bank's map, bit for
 * bit.  On any difference nothing is written and the call fails with EKF_ERR_STATE.  The slot's active bound is raised to the
 * hypothesis's.
 * Every call returns EKF_ERR_ARG for a NULL bank, a range outside it or a bad argument, with nothing changed; the message is in
 * ekf_hyp_last_error.  Not part of a bank: a STREAM of unlabelled steps inside ekf_hypotheses_run, joint compatibility per
 * hypothesis, the per-hypothesis innovation and pose logs, per-hypothesis noise.
 * ekf_hypotheses_weigh / ekf_hypotheses_resample (their errors too go to ekf_hyp_last_error) keep a bank running: the weights'
 * statistics and a systematic resampling ON THE DEVICE -- the pose rows are what moves, 393 MB at count = 4096, N = 2000.  Every
 * output of both may be NULL; a call blocks exactly when one is not, else it is asynchronous on the bank's stream like ekf_hyp_step.
 * Their scratch -- 20 bytes per hypothesis -- is allocated at the first call of either.
 * Weights: w_k ~ exp(loglik_k - max) over the hypotheses whose log-likelihood is finite and whose sticky EKF_FLAG_NONFINITE is
 * clear; the others weigh nothing.  live = the hypotheses with w_k > 0, ess = (sum w)^2 / sum w^2, logmean = max + ln sum
 * exp(loglik - max) - ln count, the bank's evidence under equal priors.  A degenerate bank (nothing weighs): ess = 0, live = 0,
 * logmean = -inf, and resampling it is the identity: nothing is written, ancestors[k] = k, offspring[k] = 1.
 * Resampling with the offset u in [0, 1): with C_k the inclusive cumulative sum of the normalised weights, t_k = clamp(ceil(count
 * C_k - u), 0, count), t = count from the last live hypothesis on, offspring[k] = t_k - t_(k-1).  Survivors stay in place
 * (ancestors[k] = k wherever offspring[k] >= 1); the i-th dead slot in ascending order takes the i-th entry of the list in which
 * each ancestor, ascending, appears offspring - 1 times: its pose, block, bound, flags, n_obs, n_rej and pose rows, bit for bit.
 * Every hypothesis's loglik becomes logmean: the weights are uniform afterwards and the evidence carries on.
 * split = s in (0, 1) makes the copies useful (deterministic filters would stay identical for ever): every slot whose ancestor has
 * two or more offspring -- the survivor too -- moves its pose mean by s L z_k (L: the lower Cholesky factor of its pose block, a
 * pivot <= 0 or not finite zeroing its column; z: count x 3 standard normal draws, the caller's) and keeps (1 - s^2) of its pose
 * block and pose rows: localize's Schmidt-Kalman update for a pose fix drawn from the ancestor's own distribution, so the
 * children's mixture has the ancestor's pose marginal and the map stays frozen.  The heading is not wrapped; no log-likelihood
 * term is added; slots of ancestors with one offspring stay bit for bit.  Refused (EKF_ERR_ARG, nothing changed): u outside
 * [0, 1) or not finite, split outside [0, 1), split > 0 with NULL or non-finite z, z given with split == 0.
 * Measured on one MI355X (tools/hyp_resample_time.py, profiles/hyp_resample.txt; N = 2000, call + sync with every output NULL):
 * count = 4096 at ess = count / 2 105 us, 182 with a split; 4095 copies of one source 114 and 250; ekf_hyp_step there: 657.
 * An uploaded stream, run with the resampling decided ON THE DEVICE (errors: ekf_hyp_last_error; every EKF_ERR_ARG leaves the bank
 * bit for bit).  ekf_hypotheses_stream_upload is ekf_hyp_step's arguments with a leading [step] axis: lin / ang [steps] (motion_stride 0)
 * or [steps][count]; idx / range / bearing [steps][stride] and m [steps] (obs_stride 0) or [steps][count][stride] and
 * [steps][count].  Every step is checked as ekf_hyp_step checks it (m <= EKF_MMAX, indices inside the map, an index may come
 * twice; as there, a range or bearing that is not finite is taken and flags the hypothesis that sees it) and packed into the
 * records a step uploads -- one per step where both strides are 0, else count, 352 B each -- which are copied to the device.
 * Blocking.  A new upload replaces the old one, steps == 0 frees it.  The map is frozen, so the stream never goes stale: resets,
 * resamplings, single steps and adoptions between runs leave it runnable.  A failed allocation returns EKF_ERR_HIP with the byte
 * count and leaves the bank usable, without a stream.
 * ekf_hypotheses_run enqueues steps [first, first + count), back to back, ASYNCHRONOUS on the bank's stream like ekf_hyp_step; u and z
 * are staged by the call (it blocks only where the previous call's staged draws have not been uploaded yet).  Per step s:
 * ekf_hyp_step's two launches on the step's records; with ess_fraction > 0 or the log on, the weights (ekf_hypotheses_weigh's
 * launch); with the log on, the mixture row; with ess_fraction > 0, ekf_hypotheses_resample's launches with the offset
 * u[s - first], the split `split` and the draws z[(s - first) * count * 3 ..], GATED ON THE DEVICE: they act only where something
 * weighs and ess < ess_fraction * count (one double product formed on the host), and otherwise leave at once and write nothing --
 * the log-likelihoods stay, the weights carry on.  The bank ends bit for bit as after ekf_hyp_step and, where ess <
 * ess_fraction * count, ekf_hypotheses_resample per step.  ess_fraction above 1 resamples at every step in which something weighs.
 * No device-side wait, no second stream, no graph: plain stream-ordered launches.  EKF_ERR_ARG: a range outside the stream,
 * ess_fraction negative or not finite, split outside [0, 1), split > 0 with ess_fraction == 0, u NULL with ess_fraction > 0 or
 * given with 0, z NULL with split > 0 or given with 0, a u outside [0, 1), a z that is not finite.  EKF_ERR_STATE: no stream.
 * ekf_hypotheses_mixture (blocking; every output may be NULL) forms on the device the bank's pose mixture sum_k w_k N(pose_k, block_k):
 * mean = (sum w x, sum w y, atan2(sum w sin theta, sum w cos theta)) over the normalised weights, cov (3 x 3, symmetric) = sum w
 * (block_k + d_k d_k^T), d_k the deviation from the mean with its heading wrapped to [-pi, pi), both over the hypotheses with
 * w > 0 only (a dead one may hold NaN); ess, logmean and live as ekf_hypotheses_weigh gives them; best = the first hypothesis
 * that weighs and has the largest log-likelihood.  Where nothing weighs: NaN, ess 0, logmean -inf, live 0, best -1.  It changes
 * nothing a later call can see.  Every sum has a fixed order: the same bank gives the same bits here and in the log.
 * ekf_hypotheses_log(capacity > 0) keeps the last `capacity` steps' rows in a device ring and restarts the count at 0; capacity 0
 * switches the log off (after a stream synchronisation).  Neither changes a bit of the bank.  Only ekf_hypotheses_run's steps write
 * rows: a row is the mixture BEHIND THE STEP'S UPDATE AND BEFORE ITS RESAMPLING -- the exact posterior summary, which a resampling
 * keeps only in expectation -- and `resampled`, whether the step's resampling acted.  ekf_hypotheses_log_steps: the steps logged.
 * ekf_hypotheses_download_log (blocking, stream-ordered; every output may be NULL): steps [first, first + count), which must be among
 * the last `capacity` logged (else EKF_ERR_ARG); EKF_ERR_STATE while the log is off.
 * Windows of RAW DETECTIONS, single and streamed (errors: ekf_hyp_last_error; every EKF_ERR_ARG leaves the bank bit for bit).  The
 * bank's tag-table row (the source slot's, copied at creation) and its map are frozen and the walk of a window reads no pose, so a
 * window is associated ONCE, on the device, for every hypothesis (k_hyp_associate: ekf_localize_detections' walk and its rules -- the
 * ignore list, the gate, ids outside [0, 1024) dropped with EKF_FLAG_ASSOC, one slot per distinct tag in order of first
 * appearance, per-tag averaging; a tag the row does not know or whose entry lies beyond the map is UNMATCHED: skipped, reported,
 * no flag; more than EKF_AMAX distinct matched tags: the surplus dropped with EKF_FLAG_ASSOC), and a tag's averaged (range,
 * bearing) has the bits ekf_localize_detections gives it.  The bank takes the handle's association settings at creation, as it
 * takes the noise pair and the NIS gate; ekf_hypotheses_set_association (ekf_set_association's argument rules) changes them for later
 * calls and uploads -- a stream already uploaded is NOT associated again.  EKF_ERR_STATE: the source slot had no tag table.
 * ekf_hypotheses_step_detections: ONE window and ONE motion for every hypothesis (the robot has one camera; per-hypothesis motion
 * stays with ekf_hyp_step), asynchronous on the bank's stream: the window's upload, the association, then ekf_hyp_step's two
 * launches on the first EKF_MMAX matched tags and, where the window holds more than EKF_MMAX distinct ids, ekf_hyp_update's on the
 * rest -- a hypothesis ends bit for bit as after ekf_hyp_step + ekf_hyp_update with the lists ekf_hypotheses_download_tags reports,
 * and a second pass that finds nothing to apply leaves every hypothesis bit for bit.  EKF_ERR_ARG: count outside [0, EKF_DMAX], NULL
 * arrays with count > 0, lin or ang not finite.
 * ekf_hypotheses_detections_upload (blocking): `steps` windows -- lin / ang / count [steps], tag_id / pose_err [steps][stride], pose_t
 * [steps][stride][3] -- copied, associated in ONE launch (a wave per window) and kept as the bank's stream with each step's matched
 * tags, unmatched ids and flag; ekf_hypotheses_run runs it exactly as it runs an index stream, with a second solve / rows pair in the
 * steps that matched more than EKF_MMAX tags (weighing, the log's row and the resampling follow the step's last pass).  It replaces
 * an earlier stream of either kind, as ekf_hypotheses_stream_upload replaces this one; steps == 0 frees it; a refused call leaves
 * the earlier stream; a failed allocation returns EKF_ERR_HIP with the byte count and leaves the bank usable, without a stream.
 * ekf_hypotheses_download_tags (blocking; every output may be NULL; the arrays hold EKF_AMAX entries): the window of `step` of the
 * uploaded detection stream, or with step == -1 the last single window -- *m matched tags in update order (landmark index, tag
 * id, averaged error, range, bearing), *n_unmatched distinct unmatched ids and the first EKF_AMAX of them (-1 beyond), and the
 * window's flag (0 or EKF_FLAG_ASSOC).  EKF_ERR_STATE if no such window exists.
 * Measured on one MI355X (tools/hyp_detections_time.py, profiles/hyp_detections.txt; N = 2000, 8 tags x 3 frames, 200 windows,
 * host-clocked): the window's upload and the association add 13 .. 14 us to a step (200 calls behind one sync against ekf_hyp_step
 * with the reported lists); one window, call + sync, against the host's association + ekf_hyp_step: 72 / 86 us at count = 32,
 * 207 / 223 at 1024, 802 / 817 at 4096; the upload of 200 windows 2.5 ms against 6.5 with the host's association; ekf_hypotheses_run
 * per step on the detection stream and on the index stream of the same lists: 23.1 / 23.1, 159.0 / 159.0, 752.3 / 752.5.
 * UNLABELLED observations, associated per hypothesis ON THE DEVICE (errors: ekf_hyp_last_error; every EKF_ERR_ARG leaves the bank
 * bit for bit).  Which landmark an observation belongs to depends on the pose, so it differs between hypotheses: k_hyp_score
 * (ekf_hyp_assoc.hip) scores, for each hypothesis, every landmark of the map against every observation of ONE list of m <=
 * EKF_MMAX (range, bearing) pairs -- the robot has one camera -- exactly as ekf_associate scores them for a slot: from the joint
 * 5 x 5 covariance of (pose, landmark) -- the hypothesis's pose block and pose rows, the map's landmark block -- S = H5 P5 H5^T +
 * Q with the bank's measurement noise, NIS = y^T S^-1 y (bearing wrapped) and the score d = NIS + ln det S, by the one function
 * both kernels call.  Per observation the two landmarks of smallest d, best first: a strictly smaller score replaces, ties stay
 * with the lower landmark index, a NaN never wins, an empty map or all-NaN scores give -1 / NaN.  A hypothesis's result depends
 * on its own state, the map and the observations, not on count, on k or on which hypotheses share the call.
 * ekf_hypotheses_associate (blocking, stream-ordered behind the bank's stream; it changes nothing a later call can see): the
 * scores of hypotheses [k0, k0 + count), shaped as ekf_associate's outputs with stride = m: cand count x m x 2, cand_nis /
 * cand_logdet count x m x 2, min_nis count x m (each of the three may be NULL), all_nis / all_logdet count x m x cap, both or
 * neither, cap >= the map's landmark count (entries beyond it: NaN).  Destinations in pinned memory (ekf_host_alloc) are written
 * directly, others through one copy each.  EKF_ERR_ARG: a range outside the bank, m outside 0..EKF_MMAX, an observation that is
 * not finite, NULL cand, all_* given singly or with a short cap.
 * ekf_hypotheses_step_unlabelled (ASYNCHRONOUS on the bank's stream): ekf_hyp_step's two launches on a prediction-only record
 * (motion_stride as there), then k_hyp_score, which also RESOLVES each hypothesis's assignment on the device and writes its step
 * record and assignment row -- nothing is downloaded --, then the bank's solve and row launches on those records (the bank's NIS
 * gate still acts inside the update).  The resolve is frontend.resolve_associations with no new landmarks (the map is frozen):
 * the observations are taken in ascending order of their best candidate's NIS (stable, NaN last); each takes its first candidate,
 * of two, that no earlier observation took, and is ACCEPTED iff that candidate's NIS <= accept (NaN compares false), else
 * DROPPED.  The accepted pairs update the hypothesis in observation order.  miss: a finite log-likelihood, normally <= 0, that
 * every dropped observation adds to the hypothesis's loglik -- the clutter term without which a hypothesis that matches nothing
 * is never penalised (evaluation.clutter_loglik gives a default): with dropped > 0 and miss != 0, loglik += dropped * miss (one
 * product, one addition) before the update's solve runs; otherwise loglik is not written by the scoring.  n_obs / n_rej count
 * only what the update then sees.  ekf_hypotheses_update_unlabelled is the same call without the prediction.  With the
 * measurement model off the observations are ignored, as ekf_hyp_update ignores them.  EKF_ERR_ARG: lin, ang or an observation
 * not finite, m outside 0..EKF_MMAX, accept negative or NaN (INFINITY: every candidate is accepted), miss not finite.
 * THE GUARANTEE: after ekf_hypotheses_step_unlabelled every hypothesis is BIT FOR BIT what it is after ekf_hyp_step with m = 0,
 * then ekf_hypotheses_associate, then frontend.resolve_associations with create = +inf on the host from the downloaded rows,
 * then ekf_hyp_update with the resulting per-hypothesis lists -- with miss = 0 including loglik, n_obs, n_rej, flags and bound --
 * and the downloaded assignment equals the host's.
 * ekf_hypotheses_download_assignment (blocking): rows [k0, k0 + count) of the last unlabelled step's assignment, EKF_MMAX ints
 * each: the landmark of every accepted observation, -1 for dropped ones and beyond m; kept until the next unlabelled call.
 * EKF_ERR_STATE before the first unlabelled step.  The records (352 B per hypothesis), the assignment rows and the query's staging
 * buffer are allocated at first use; a failed allocation returns EKF_ERR_HIP with the byte count and leaves the bank usable.
 * Measured on one MI355X (tools/hyp_associate_time.py, profiles/hyp_associate.txt; N = 2000, m = 8, us, count = 32 / 1024 / 4096):
 * ekf_hypotheses_associate call + sync 266 / 359 / 1037; k_hyp_score alone, between an event pair, 186 / 267 / 844;
 * ekf_hypotheses_step_unlabelled per step over 200 steps behind one sync 233 / 453 / 1620, ekf_hyp_step with the true ids there
 * 28 / 138 / 620; one step + sync 251 / 475 / 1665 against 731 / 11 661 / 50 723 for the host sequence of the guarantee. */
typedef struct ekf_hypotheses ekf_hypotheses;
int ekf_hyp_create(ekf_handle *h, int b, int count, ekf_hypotheses **out);
int ekf_hyp_destroy(ekf_hypotheses *hy);
int ekf_hyp_reset(ekf_hypotheses *hy, int k0, int count, const double *pose /* count x 3 */, const double *cov /* count x 9 */);
int ekf_hyp_step(ekf_hypotheses *hy, const double *lin, const double *ang, int motion_stride, const int *idx,
                 const double *range, const double *bearing, const int *m, int stride, int obs_stride);
int ekf_hyp_update(ekf_hypotheses *hy, const int *idx, const double *range, const double *bearing, const int *m, int stride,
                   int obs_stride);
int ekf_hyp_download(ekf_hypotheses *hy, int k0, int count, double *pose, double *cov /* count x 9 */, double *loglik,
                     long long *n_obs, long long *n_rej, unsigned *flags);
int ekf_hyp_download_rows(ekf_hypotheses *hy, int k, double *rows /* 3 x n */, int n);
int ekf_hyp_set_nis_gate(ekf_hypotheses *hy, double threshold);
int ekf_hyp_adopt(ekf_hypotheses *hy, int k, ekf_handle *h, int b);
int ekf_hyp_sync(ekf_hypotheses *hy);
const char *ekf_hyp_last_error(ekf_hypotheses *hy);
int ekf_hypotheses_weigh(ekf_hypotheses *hy, double *ess, double *logmean, int *live);
int ekf_hypotheses_resample(ekf_hypotheses *hy, double u, double split, const double *z /* count x 3, or NULL iff split == 0 */,
                            int *ancestors /* count */, int *offspring /* count */, double *ess, double *logmean);
int ekf_hypotheses_stream_upload(ekf_hypotheses *hy, int steps, const double *lin, const double *ang, int motion_stride,
                          const int *idx, const double *range, const double *bearing, const int *m, int stride, int obs_stride);
int ekf_hypotheses_run(ekf_hypotheses *hy, int first, int count, double ess_fraction, double split,
                const double *u /* count, NULL iff ess_fraction == 0 */, const double *z /* count x K x 3, NULL iff split == 0 */);
int ekf_hypotheses_mixture(ekf_hypotheses *hy, double *mean /* 3 */, double *cov /* 9 */, double *ess, double *logmean, int *live, int *best);
int ekf_hypotheses_log(ekf_hypotheses *hy, int capacity);
int ekf_hypotheses_log_steps(ekf_hypotheses *hy, long long *logged);
int ekf_hypotheses_download_log(ekf_hypotheses *hy, long long first, int count, double *mean /* count x 3 */, double *cov /* count x 9 */,
                         double *ess, double *logmean, int *live, int *best, int *resampled);
int ekf_hypotheses_set_association(ekf_hypotheses *hy, double gate_range, const int *ignore_tags, int n_ignore);
int ekf_hypotheses_step_detections(ekf_hypotheses *hy, double lin, double ang, int count,
                                   const int *tag_id, const double *pose_t /* count x 3 */, const double *pose_err);
int ekf_hypotheses_detections_upload(ekf_hypotheses *hy, int steps, const double *lin, const double *ang, const int *count,
                                     const int *tag_id, const double *pose_t, const double *pose_err, int stride);
int ekf_hypotheses_download_tags(ekf_hypotheses *hy, int step /* -1: the last single window */, int *m, int *idx, int *tag_id,
                                 double *err, double *range, double *bearing, int *n_unmatched, int *unmatched /* EKF_AMAX */,
                                 unsigned *flags);
int ekf_hypotheses_associate(ekf_hypotheses *hy, int k0, int count, const double *range, const double *bearing, int m,
                             int *cand, double *cand_nis, double *cand_logdet, double *min_nis,
                             double *all_nis, double *all_logdet, int cap);
int ekf_hypotheses_step_unlabelled(ekf_hypotheses *hy, const double *lin, const double *ang, int motion_stride,
                                   const double *range, const double *bearing, int m, double accept, double miss);
int ekf_hypotheses_update_unlabelled(ekf_hypotheses *hy, const double *range, const double *bearing, int m,
                                     double accept, double miss);
int ekf_hypotheses_download_assignment(ekf_hypotheses *hy, int k0, int count, int *assign /* count x EKF_MMAX */);

/* Streams of pre-uploaded inputs ([step][batch] and [step][batch][stride] arrays, stride <= EKF_MMAX; m[step][batch] landmarks
 * each -- any count per step and trajectory, 0 included: what the windows of src/replay_no_ros.py:280-301 hold).
 * ekf_stream_upload copies and validates `steps` steps of inputs into HBM (blocking);
 * ekf_stream_run enqueues steps [first, first+count) back to back (asynchronous).  Where nothing is pending they run as packed
 * cadences ("fused_cadence"): per covariance pass every trajectory's next 40 landmark updates, whatever steps they belong to --
 * inside the call the trajectories of a bank advance through the range at their own pace (they are independent filters); when
 * the call returns every one of them has been enqueued up to first+count;
 * ekf_run_stream = upload + run all.
 * Driving a stream in SHORT pieces: a cadence only forms where nothing is pending, and a call's last cadence leaves its ranks
 * pending unless its 40 slots are used up (right for one long run, and for online steps behind it) -- the next call then runs the
 * per-step kernels until the pass is due, so the "40 landmark updates per pass" only hold for long calls.  With
 * ekf_set_option("run_end_flush", 1) every call ends with the covariance pass of what it left pending and every piece runs
 * fused (one pass per call: worth it from ~40 landmark updates per call).  The plan of a call's cadences is made and uploaded
 * per call (32 B per cadence and trajectory). */
int ekf_stream_upload(ekf_handle *h, int steps, const double *lin, const double *ang, const int *idx,
                      const double *range, const double *bearing, const int *m, int stride);
int ekf_stream_run(ekf_handle *h, int first, int count);
int ekf_run_stream(ekf_handle *h, int steps, const double *lin, const double *ang, const int *idx,
                   const double *range, const double *bearing, const int *m, int stride);

/* General dense propagation P <- F P F^T + Q (F, Q row-major n x n) on the fp64 MFMA path: the
 * reference's literal G_F @ P @ G_F.T + F.T @ R @ F product (src/replay_no_ros.py:430) for an
 * arbitrary Jacobian. */
int ekf_predict_dense(ekf_handle *h, int b, const double *F, const double *Q);

/* The covariance is held as P_base + (pending low-rank update of the last few steps, 2 ranks per observed
 * landmark -- exactly: a step is charged the ranks of its busiest trajectory, whatever the landmark count); the O(n^2) pass over
 * P_base is paid once per `flush_every` steps (option; default 0 = as many landmark updates as fit `rank_limit` = 80 pending
 * ranks: 40 -- 5 steps at 8 observations per step, 8 at five, 40 at one).  ekf_flush
 * applies what is pending now (asynchronous).  Every call that reads or rewrites the covariance flushes by
 * itself. */
int ekf_flush(ekf_handle *h);
/* Wait for everything enqueued.  EKF_ERR_STATE if any trajectory carries EKF_FLAG_INTERNAL (ekf_last_error names it). */
int ekf_sync(ekf_handle *h);
/* The sticky flags of trajectory b (always EKF_OK for a valid b: this is how a failed trajectory is identified). */
int ekf_status_flags(ekf_handle *h, int b, unsigned *flags);

/* Message of the last failure on this handle (h == NULL: last failure of ekf_create). */
const char *ekf_last_error(ekf_handle *h);

/* --- measurement hooks (HIP events on the handle's own stream) --- */
int ekf_timer_begin(ekf_handle *h);
int ekf_timer_end(ekf_handle *h, double *elapsed_ms);          /* synchronises */
/* When enabled every launch of the covariance pass (flush) kernel is bracketed by an event pair -- every k-th one with
 * ekf_set_option("profile_stride", k): an event record costs its stream ~6 us, which a single trajectory's 80 us cadence
 * feels.  ekf_profile_read: total time and number of the BRACKETED launches (and resets); ekf_profile_passes: all launches of
 * the pass since profiling was enabled, bracketed or not. */
int ekf_profile_enable(ekf_handle *h, int on);
int ekf_profile_read(ekf_handle *h, double *pass_ms_total, long long *pass_launches); /* and resets */
long long ekf_profile_passes(ekf_handle *h);
/* With ekf_set_option("profile_kernels", 1) (a diagnostic run: every record costs its stream ~6 us) the other launches of a
 * fused cadence carry event pairs too: cls 1 the solve launch, 2 the chain (or look-ahead gather) launch, 3 the panel launch,
 * 0 the pass; 4 the k_direct launch of ekf_update_direct; 5 the k_linear launch of ekf_update_linear; 6 the k_join launch of ekf_join_maps (with its snapshot launch); 7 the k_predict_pose launch of ekf_predict_linear; 8 the k_transform launch of ekf_transform; 9 and 10 the k_loc_solve and k_loc_rows launches of ekf_localize_*; 11 the k_loc_associate launch of ekf_localize_detections.  Does not reset: read before ekf_profile_read. */
int ekf_profile_read_class(ekf_handle *h, int cls, double *ms_total, long long *launches);
/* Options: name (default, allowed values) meaning.  Unknown names and values out of range fail with EKF_ERR_ARG.
 *   "flush_every"         (0, 0..64)    steps per covariance pass; 0 = auto, by "rank_limit"
 *   "rank_limit"          (80, 2..80)   auto cadence: pending ranks that trigger the pass
 *   "pass_kernel"         (-1, -1/0/2)  covariance pass: -1 auto, 0 column strips (k_flush), 2 row slabs (k_flush_rs); same bits
 *   "pass_chunk"          (0, 0..4096)  row-slab pass: strips per work unit, 0 = auto
 *   "pass_workgroups"     (0, 0..4096)  row-slab pass: persistent workgroups, 0 = one per CU (fewer leave CUs to other streams)
 *   "pass_rows_per_block" (0, 0..4096)  column-strip pass: rows per workgroup (multiple of 16), 0 = auto
 *   "pass_streaming"      (-1, -1..1)   -1 auto by working-set size, 0 resident, 1 nontemporal
 *   "active_bound"        (1, 0..1)     0 = treat every state index as correlated (flushes first)
 *   "small_state"         (1, 0..1)     1 = n_max <= 79 (<= 131 for banks of >= 128) runs as one workgroup per trajectory with P
 *                                       in LDS, nothing ever pending; env EKFSLAM_HIP_SMALL_STATE sets it for new handles (flushes first)
 *   "fused_step"          (1, 0..2)     1 = small launches run a step as one kernel, 0 = always two; 2 = diagnostic: the solve never
 *                                       publishes its completion, every bounded wait times out with EKF_FLAG_INTERNAL
 *   "fused_cadence"       (1, 0..1)     1 = ekf_stream_run runs everything between two passes (a trajectory's next 40 landmark
 *                                       updates and the predictions between them) as one solve + one panel launch; equal to the
 *                                       per-step kernels to rounding (the tests assert 1e-11); 0 = one step at a time
 *   "col_gather"          (1, 0..1)     1 = the panel launch's mirrored column entries are gathered beside the solve; same bits
 *   "w_from_v"            (1, 0..1)     1 = a row-slab pass right behind the panel launch forms W from V and the records, the panel
 *                                       launch writes V only; same bits (ekf_debug_snapshot's W view is then stale)
 *   "panel_shape"         (0, 0..3)     diagnostics: 0 = the panel launch's shape by its size, 1 .. 3 force row-split / one wave /
 *                                       four waves per workgroup; same bits
 *   "lookahead"           (1, 0..1)     1 = where the pass is a small launch, the next cadence's solve runs beside it
 *   "chain"               (1, 0..1)     1 = banks of up to 40 whose pass leaves CUs free chain their solves on the handle's stream,
 *                                       panel launch and pass on the second one, at every size; 0 = the round-3 look-ahead, from
 *                                       48 MB of covariance.  Set 0 under rocprofv3 --pmc or any kernel-serialising profiler
 *   "panel_tform"         (1, 0..1)     chained runs: small panel launches as a triangular solve on the matrix cores
 *   "run_end_flush"       (0, 0..1)     1 = every ekf_stream_run call ends with the pass of what it left pending
 *   "pack_dense"          (1, 0..2)     downloads into pinned memory: 1 = a kernel writes up to 40 MB straight into the destination,
 *                                       2 = at every size, 0 = never (mirror pass + copy); same bytes
 *   "fetch_spin"          (1, 0..1)     ekf_step_fetch on the small-state path polls the sequence word its launch releases behind
 *                                       the state in pinned memory (the ordering this assumes: INTEGRATION.md section 3), 0 =
 *                                       waits for the stream; env EKFSLAM_HIP_FETCH_SPIN sets it for new handles
 *   "fetch_verify"        (1, 0..1)     1 = a polled hand-over is trusted only if the XOR checksum of its payload matches (~1 us);
 *                                       0 = the second sequence number only.  A mismatch waits for the stream (ekf_debug_fetch_retries)
 *   "profile_kernels"     (0, 0..1)     measurement: event pairs around every launch of a fused cadence (ekf_profile_read_class)
 *   "profile_stride"      (1, 1..1024)  measurement: every k-th pass launch carries an event pair
 * "fused_cadence", "lookahead" and "chain" change the ORDER in which a step's pending ranks are summed (and whether the
 * look-ahead applies depends on the device's CU count and the size of the launch): results are equal to rounding across these
 * settings and across devices, bit-identical only for a fixed setting on a fixed device type. */
int ekf_set_option(ekf_handle *h, const char *name, int value);
/* Which form of the covariance pass the last launch used (-1 = none yet; values as for "pass_kernel"), how many
 * MFMA k-tiles (4 pending ranks each) it applied, and whether it took the nontemporal (streaming) path. */
int ekf_last_pass(ekf_handle *h, int *kernel, int *k_tiles, int *streaming);

/* --- diagnostics (development hooks: counters and raw views the tests use to assert WHICH path ran; no reference
 * interface stands behind them, they change nothing, and a production caller never needs them) --- */
/* Fused cadences ekf_stream_run has launched so far and the steps (of the uploaded stream) they covered. */
int ekf_debug_cadences(ekf_handle *h, long *cadences, long *steps);
/* Host fallbacks of the device-side association: a binding whose window does not fit the device front end's limits takes the
 * host association instead and says so with ekf_debug_note_assoc_fallback; ekf_debug_assoc_fallbacks returns the count. */
long ekf_debug_assoc_fallbacks(ekf_handle *h);
void ekf_debug_note_assoc_fallback(ekf_handle *h);
/* Cadences whose solve ran beside the previous covariance pass (chained solves or look-ahead), and how many of those had
 * their block formed from the previous cadence's records (chained solves, option "chain"). */
long ekf_debug_lookaheads(ekf_handle *h);
long ekf_debug_chained(ekf_handle *h);
/* Covariance passes that formed their W fragments from V and the cadence's records (option "w_from_v"). */
long ekf_debug_w_from_v(ekf_handle *h);
/* ... and whether the last pass was one of them (the fourth template argument of k_flush_rs in a profiler's listing). */
int ekf_debug_last_pass_wv(ekf_handle *h);
/* Pieces of the longest static share the last row-slab pass used (0 = work queues / column strips; -1 = NULL handle). */
int ekf_debug_last_pass_shares(ekf_handle *h);
/* Launches of the small-state path; ekf_step_fetch calls served by the step's own launch; whole-state downloads written
 * by k_pack_dense. */
long ekf_debug_small_launches(ekf_handle *h);
long ekf_debug_fused_fetches(ekf_handle *h);
long ekf_debug_dense_packs(ekf_handle *h);
/* ekf_step_fetch hand-overs whose integrity trailer did not match what the host polled (answered after a stream
 * synchronisation instead): 0 on a platform where the ordering assumption of the polled hand-over holds. */
long ekf_debug_fetch_retries(ekf_handle *h);
/* Raw device views behind a stream synchronisation, no flush: the fused cadence's record of trajectory b (returns its
 * size; copies min(bytes, size)); `which` = 0 P_base (allocated doubles), 1 V, 2 W, 3 the mean buffer the next step reads,
 * 4 the other mean buffer, 5 (chained runs, every trajectory: b is ignored) the mean at the positions of the last chained
 * cadence, 128 doubles per trajectory (dst == NULL: the count). */
long ekf_debug_cad(ekf_handle *h, int b, void *dst, long bytes);
long ekf_debug_snapshot(ekf_handle *h, int b, int which, double *dst, long count);
/* The planning arithmetic of the row-slab pass, host side only (no handle, no device): every unit of the eight per-XCD
 * work queues in hand-out order (returns their number), and the static shares (workgroups x 16 pieces x 4 ints; returns the
 * pieces of the longest share, 0 if one would need more than 16). */
int ekf_debug_pass_units(int batch, int nrb, int nch, int mode, int *out, int cap);
int ekf_debug_pass_shares(int batch, int n_hi, int workgroups, int *out);
/* k_hyp_score alone (tools/hyp_associate_time.py): `reps` launches of ekf_hypotheses_associate's query over the whole bank --
 * candidates only, into the query's staging buffer, nothing copied back -- between one event pair on the bank's stream;
 * *us_per_launch: the pair's time / reps in microseconds.  Blocking; changes nothing of the bank.  The arguments are checked as
 * the query's; reps >= 1. */
int ekf_debug_hyp_score_time(ekf_hypotheses *hy, const double *range, const double *bearing, int m, int reps, double *us_per_launch);

#ifdef __cplusplus
}
#endif
#endif
