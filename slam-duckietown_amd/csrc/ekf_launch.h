// The launch boundary: every launch_* function ekf_api.hip calls, declared once and included by the .hip file that defines it.
// The launchers take named views of the handle (ekf_device.h: BankView, StepBufs, PendingView) plus what only they need, and
// unpack them on the host into the kernel's arguments; no kernel takes a view.
#pragma once
#include "ekf_device.h"

namespace ekf {
struct PassPlan; struct RemovePlan; struct HypResamplePlan;   // ekf_host_plan.h
// ---- per-step kernels (ekf_kernels.hip) ----
// What a step's solve takes beside the views; the single-launch step also the handle's dmbox (throughput shape), dready, step_seq
struct StepArgs {
  const StepIn* in; double* fac; const int* neff_floor; int kbase;
  SolveOut* mbox = nullptr; unsigned* ready = nullptr; unsigned seq = 0; int publish = 0;
};
void launch_solve(hipStream_t st, const BankView& k, const StepBufs& s, const StepArgs& a, const DeviceConfig& cfg);
void launch_step_split(hipStream_t st, int mcap, const BankView& k, const StepBufs& s, const StepArgs& a, const DeviceConfig& cfg, int n_hi);
void launch_step_split_tp(hipStream_t st, int mcap, const BankView& k, const StepBufs& s, const StepArgs& a, const DeviceConfig& cfg,
                          int n_hi);   // the throughput shape of the single-launch step: k_panels<.., SPLIT> (see there)
// `latency` (ekf_host_plan.h: plan_step): four waves split the pending ranks of 64 indices; else the throughput form, a
// workgroup is four independent waves of 64 state indices sharing one staging
void launch_panels(hipStream_t st, int mcap, bool latency, const BankView& k, const StepBufs& s, const double* fac, int n_hi);
void launch_predict_rc(hipStream_t st, const BankView& k, const StepBufs& s, int n_hi);
// p.streaming = the batch's covariances do not fit the Infinity Cache: nontemporal accesses
void launch_flush(hipStream_t st, const PassPlan& p, const BankView& k, const double* dacc);
// the row-slab form of the pass (k_flush_rs): persistent workgroups, k.queue = 8 x RS_QSTRIDE zeroed words; the work queues'
// hand-out as planned (plan_pass), or one equal static share per workgroup (mode 4) where `shares` is given; wv: w_from_v
void launch_flush_rs(hipStream_t st, const PassPlan& p, const BankView& k, const double* dacc, const int* shares, const CadOut* wv);
int flush_rs_queue_words();
// one trajectory: Pb, mub, flag_b are its covariance, mean and flags word
void launch_add_landmarks(hipStream_t st, double* Pb, double* mub, int ld, int n_old, int n_new, double var, const double* xy);
void launch_fill_diag(hipStream_t st, double* Pb, int ld, int n, const double* diag);
void launch_mirror(hipStream_t st, double* P, const int* nact, int ld, long pstride, int batch, int n_hi);
void launch_pack_small(hipStream_t st, const double* Pb, const double* mub, const unsigned* flag_b, int ld, int n, double* host_out);
void launch_pack_dense(hipStream_t st, const double* Pb, int ld, int n, double* host_out);
// ---- the small-state path (ekf_small.hip) ----
// ekf_step_fetch: trajectory out_b's state goes to the pinned host_out, released by out_seq in *host_seq (out_b < 0: none)
struct SmallFetch {
  double* host_out = nullptr; int out_b = -1;
  unsigned long long* host_seq = nullptr; unsigned long long out_seq = 0;
};
// form: ekf_host_plan.h's SmallForm (plan_small); lg / plg: the logging instantiations.  Non-zero: hipFuncSetAttribute failed.
int launch_small_stream(hipStream_t st, const BankView& k, const StepBufs& s, const StepIn* in, int nsteps, const DeviceConfig& cfg,
                        int n_hi, int form, const SmallFetch& f, const InnovLog* lg, const PoseLog* plg);
// ---- fused cadences (ekf_cadence.hip) ----
long cadence_gbuf_doubles();   // per trajectory: CAD_GP parts
int chain_sync_words();
// (look-ahead) the next cadence's block while `kb` ranks and the noise `dacc` are pending -> gbuf
void launch_gather_cad(hipStream_t st, const BankView& k, const double* dacc, const StepIn* in, const CadPlan* plan, int kb,
                       const DeviceConfig& cfg, double* gbuf);
// `colbuf` (batch x CAD_CU x ld doubles, or nullptr): the launch also gathers the mirrored column entries of the panel launch
// behind it, on `col_wgs` extra workgroups -- only where P_base is current (not beside a pass: look-ahead)
// `chain`: the instantiation that also records the pose block behind the cadence (CadOut::posefin) for k_chain_cad; `gmu`
// (with gbuf, one part): block and mean come from k_chain_cad.  Writes s.mu_out, s.dacc_out and the records s.cad.
struct SolveCadArgs {
  const double* gbuf = nullptr; int gparts = 0;
  double* colbuf = nullptr; int col_wgs = 0;
  bool chain = false;
  const double* gmu = nullptr; unsigned* sync = nullptr; unsigned start_sigma = 0; const CadPre* pre = nullptr;
};
void launch_solve_cad(hipStream_t st, const BankView& k, const StepBufs& s, const StepIn* in, const CadPlan* plan,
                      const DeviceConfig& cfg, int n_hi, const SolveCadArgs& a, const PoseLog* plg);
// (chained runs) the next cadence's block and mean from cadence `prev`, whose solve has just run: its records prev.cad, the mean
// it read (prev.mu_in: the landmarks) and left the pose in (prev.mu_out), the pose rows before it (prev.prow3_in).  `plan`: the
// next cadence's; `gw` gather workgroups per trajectory (ekf_host_plan.h: chain_gather_workgroups); pre_out / plan2: the inputs
// of the cadence after the next, formed ahead (nullptr: none follows)
struct ChainArgs {
  double *gbuf, *gmu, *xg, *bg;
  unsigned* sync; unsigned sigma = 0, gather_target = 0; int gw = 1; bool wait_pass = false;
  const CadPre* pre_in = nullptr; CadPre* pre_out = nullptr; const CadPlan* plan2 = nullptr;
};
void launch_chain_cad(hipStream_t st, const BankView& k, const StepBufs& prev, const StepIn* in, const CadPlan* plan,
                      const DeviceConfig& cfg, const ChainArgs& a);
void launch_mark(hipStream_t st, unsigned* sync, unsigned sigma);
void launch_gate(hipStream_t st, unsigned* sync, unsigned sigma, unsigned* flags, int batch);
void launch_snap_pose(hipStream_t st, const BankView& k, int n_hi, double* prow3);
// `nrp`: the ranks the bank's busiest trajectory appends, padded to a whole k-tile (every trajectory writes that many);
// `form`: ekf_host_plan.h's PanelForm (plan_cadence_step); `skipw` (w_from_v): the replay forms write V only; sync / tail_target /
// start_sigma: a chained cadence's hand-overs.  Reads the records s.cad, leaves the pose rows in s.prow3_out (nullptr: not kept).
struct PanelCadArgs {
  int nrp, form; bool skipw; const double* colbuf;
  unsigned* sync = nullptr; unsigned tail_target = 0, start_sigma = 0;
};
void launch_panels_cad(hipStream_t st, const BankView& k, const StepBufs& s, int n_hi, const PanelCadArgs& a);
// ---- the logs (ekf_innovations.hip, ekf_pose_log.hip) ----
void launch_innov_step(hipStream_t st, const StepIn* in, const SolveOut* so, int meas, int gate, int batch, const InnovLog& lg);
void launch_innov_cad(hipStream_t st, const StepIn* in, const CadPlan* plan, const CadOut* co, int meas, int gate, int batch,
                      const InnovLog& lg);
void launch_pose_step(hipStream_t st, const PendingView& f, const PoseLog& lg);
// ---- the read-only queries (ekf_marginals.hip, ekf_associate.hip, ekf_joint.hip) ----
void launch_marginals(hipStream_t st, const PendingView& f, int cap, double* pose_out, double* lm_out);
long assoc_query_part_doubles(int count, int chunks, int stride);
void launch_assoc_query(hipStream_t st, const PendingView& f, const DeviceConfig& cfg, int stride, int cap, int chunks,
                        const double* zr, const double* zb, const int* zm, double* part, double* all_nis, double* all_logdet,
                        int* cand, double* cand_nis, double* cand_logdet, double* min_nis);
void launch_joint(hipStream_t st, const PendingView& f, int ns, int nt, int tiles, const int* sel, double* mean_out, double* cov_out);
// ---- the covariance's Cholesky factor (ekf_factor.hip) ----
// every launch of the blocked factorisation of trajectories [f.b0, f.b0 + f.count) into w: the load, then per block step the
// diagonal block, the row panel and the trailing down-date; nblk_hi: blocks of the range's largest state (plan_factor)
void launch_factor(hipStream_t st, const PendingView& f, const FactorView& w, int nblk_hi);
// trajectories [f0, f0 + count) OF THE FACTORED RANGE, nblk_hi the blocks of their largest state; x (the right-hand sides: the
// solve updates them in place) / z, white / out: [count][nrhs][stride] on the device, quad [count][nrhs]
void launch_factor_solve(hipStream_t st, const FactorView& w, int f0, int count, int nblk_hi, double* x, int nrhs, int stride,
                         double* white, double* quad);
void launch_factor_multiply(hipStream_t st, const FactorView& w, int f0, int count, int nblk_hi, const double* z, int nrhs,
                            int stride, double* out);
// ---- state surgery (ekf_remove.hip, ekf_direct.hip, ekf_linear.hip, ekf_predict_linear.hip, ekf_localize.hip, ekf_loc_assoc.hip, ekf_hypotheses.hip, ekf_copy.hip, ekf_join.hip, ekf_transform.hip, ekf_dense.hip) ----
// rp.rows: the launch's largest new size (grid rows); nb trajectories from b0; src / dst: rp's tables on the device
void launch_remove(hipStream_t st, const BankView& k, double* mu, const RemovePlan& rp, const int* src, const int* dst,
                   unsigned* rflag, int b0, int nb, unsigned seq);
// the rank fronts: rows_cap = front_rows_cap(kpad, DIRECT_ROWS / LINEAR_ROWS); plan, meas, out: the parts of the launch's FrontTable
void launch_direct(hipStream_t st, int rows_cap, const BankView& k, double* dacc, double* mu, const int* plan, const double* meas,
                   double* out, int kpad);
// nsl = 3 + 2 * lstride, the columns of the call's H; meas: linear_dbls(rows_cap, nsl) per trajectory
void launch_linear(hipStream_t st, int rows_cap, const BankView& k, double* dacc, double* mu, const int* plan, const double* meas,
                   double* out, int kpad, int nsl, int innovation);
// trajectories [f.b0, f.b0 + f.count), one record each in `in`; P and mu: f.P and f.mu, written (rows 0..2 and the pose mean);
// n_hi: the largest bound of a record that applies (plan_predict_linear); f.kb > 0: the form that gathers the pending ranks
void launch_predict_pose(hipStream_t st, const PendingView& f, double* P, double* mu, const PredictIn* in, int n_hi);
// ekf_localize_* (ekf_localize.hip): the whole bank, one StepIn each in `in` (device copy, uploaded stream or the pinned ring).
// The solve writes the pose mean into `mu` in place, the pose block into k.P, the records `rec` (one per trajectory of the bank)
// and, for the logs, k.so[b].it[j].y / .si, k.so[b].rej and k.so[b].neff; the row launch, behind it on the same stream, applies
// the records to rows 0..2 of k.P: `groups` column groups (ekf_host_plan.h: loc_rows_groups of the bank's largest bound)
void launch_loc_solve(hipStream_t st, const BankView& k, double* mu, const StepIn* in, const int* neff_floor, LocRec* rec,
                      const DeviceConfig& cfg);
void launch_loc_rows(hipStream_t st, const BankView& k, const LocRec* rec, int groups);
// ekf_step_detections (ekf_loc_assoc.hip): the whole bank, one DetIn each in `det`; writes the tag table, k.nact, the new landmarks'
// means in `mu`, their rows / columns of k.P (zeros in k.V / k.W for the pending_k ranks), step_out, assoc_out, neff_dev, k.flags
void launch_associate(hipStream_t st, const BankView& k, const DetIn* det, int* tagmap, int* neff_dev, double* mu, StepIn* step_out,
                      AssocOut* assoc_out, const AssocConfig& cfg, int n_max, int pending_k);
// ekf_localize_detections (ekf_loc_assoc.hip): the whole bank, one DetIn each in `det`; reads tagmap, k.nact and the pose in `mu`,
// writes step_out[b] and step_out[k.batch + b] (what the two launch_loc_solve of the call read), assoc_out[b], unmatched[b],
// neff_dev[b] (raised over the matched landmarks) and k.flags -- nothing else
void launch_loc_associate(hipStream_t st, const BankView& k, const DetIn* det, const int* tagmap, int* neff_dev, const double* mu,
                          StepIn* step_out, AssocOut* assoc_out, LocUnmatched* unmatched, const AssocConfig& cfg);
// a hypothesis bank's windows (grid = windows, det[w] each) against the bank's tag-table row: writes step_out[w] and
// step_out[windows + w] (the shared records the bank's solves read with rec_stride 0), assoc_out[w], unmatched[w] and flags[w]
// -- nothing of the bank itself
void launch_hyp_associate(hipStream_t st, const HypView& v, const int* tagrow, const DetIn* det, int windows, StepIn* step_out,
                          AssocOut* assoc_out, LocUnmatched* unmatched, unsigned* flags, const AssocConfig& cfg);
// ---- the hypothesis bank (ekf_hypotheses.hip); v: the bank (ekf_device.h: HypView), every shape from ekf_host_plan.h's plan_hyp_* ----
// one StepIn for all hypotheses (rec_stride 0) or one each (1); the solve leaves v.rec, the row launch behind it applies them
void launch_hyp_solve(hipStream_t st, const HypView& v, const StepIn* in, int rec_stride, const DeviceConfig& cfg, bool gate);
void launch_hyp_rows(hipStream_t st, const HypView& v, int groups);
// hypotheses [k0, k0 + count): init = nullptr seeds them from the map copy's pose part, else count x 12 doubles {pose, cov}
void launch_hyp_fill(hipStream_t st, const HypView& v, const double* init, int k0, int count, int groups, int bound0);
// the bank's map against a slot's P_base / mean (layout ldb): *mismatch += entries whose bits differ
void launch_hyp_compare(hipStream_t st, const HypView& v, const double* Pb, const double* mub, int ldb, int groups, unsigned* mismatch);
void launch_hyp_adopt(hipStream_t st, const HypView& v, int k, double* Pb, double* mub, int ldb, SolveOut* so_b, int bound, int groups);
// weights, resampling and split (rs: ekf_device.h: HypResampleView; rp: plan_hyp_resample's).  weigh leaves rs.head and rs.w;
// plan reads them and leaves rs.anc / rs.off; copy and split read those and the header -- a degenerate bank is left alone
void launch_hyp_weigh(hipStream_t st, const HypView& v, const HypResampleView& rs, int chunk);
void launch_hyp_plan(hipStream_t st, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp);
void launch_hyp_copy(hipStream_t st, bool nt, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp);
// z: count x 3 draws on the device
void launch_hyp_split(hipStream_t st, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp, const double* z);
// behind weigh: the bank's mixture pose into *row; row->resampled: whether rp.ess_min's gate is open on this header
void launch_hyp_mixture(hipStream_t st, const HypView& v, const HypResampleView& rs, const HypResamplePlan& rp, HypMixRow* row);
// ---- a bank's unlabelled observations (ekf_hyp_assoc.hip) ----
// hypotheses [k0, k0 + count) against the m observations zr / zb (device; one list for all); chunks: plan_hyp_associate's.  o
// (ekf_device.h: HypScoreOut) chooses the mode: the query's outputs, or the records and assignment rows launch_hyp_solve reads
// behind it with rec_stride 1 -- then st[k].loglik is the one thing of the bank the launch writes
void launch_hyp_score(hipStream_t st, const HypView& v, const DeviceConfig& cfg, int k0, int count, int chunks, const double* zr,
                      const double* zb, int m, const HypScoreOut& o);
// groups x (tiles of the largest source + 1) workgroups; tab: plan_copy's table on the device
void launch_copy_traj(hipStream_t st, bool nt, const BankView& src, const BankView& dst, const double* mus, double* mud,
                      const int* tab, int groups, int n_hi);
// pairs x (tiles_hi + 1) workgroups behind, in sequential mode, the snapshot of the destinations' pose rows into `snap`
// (join_snap_doubles per pair; explicit mode: the host has uploaded the heads); tab: plan_join's table on the device
void launch_join(hipStream_t st, const BankView& src, const BankView& dst, const double* mus, double* mud, const int* tab,
                 double* snap, int pairs, int tiles_hi, int na_hi, bool seq);
// count x (tiles_hi + 1) workgroups, in place on k.P and mu; tab: plan_transform's table on the device, frames: count x
// transform_frame_doubles(k.ld) doubles -- the plan's heads, then k.ld means per trajectory as they stood before the call;
// nt: nontemporal stores of the 2 x 2 blocks
void launch_transform(hipStream_t st, bool nt, const BankView& k, double* mu, const int* tab, const double* frames, int count, int tiles_hi);
int dense_propagate(hipStream_t st, double* P, double* tmp, const double* F, const double* Q, int n, int ld);
}  // namespace ekf
