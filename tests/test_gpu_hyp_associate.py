"""GPU: a hypothesis bank's unlabelled observations -- ekf_hypotheses_associate, ekf_hypotheses_step_unlabelled /
_update_unlabelled, ekf_hypotheses_download_assignment (HypothesisBank.associate / step_unlabelled / update_unlabelled /
assignments; k_hyp_score, csrc/ekf_hyp_assoc.hip).

The query is compared bit for bit with EkfSlam.associate on slots that adopted the hypotheses (both kernels call one scoring
function), and judged against the NumPy reference on each hypothesis's dense state by tests/hyp_assoc_model.py with
tests/assoc_world.py's tolerances -- NIS within 1e-9 cond(S) relative, ln det S within 2e-9 cond(S) absolute -- and NO excuse:
tests/test_hyp_assoc_cpu.py holds that the table has no entry near the wrap and no unclear candidate order.  A step from unlabelled
observations is compared bit for bit with the host route of the header's guarantee: step with m = 0, associate, frontend's resolve,
update with the resulting lists."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import hyp_assoc_model as ham
from tests import hyp_support as hs
from tests import hypotheses_model as hm
from tests import resample_model as rm
from tests.conftest import path_ran
from tests.gpu_support import sd  # noqa: F401

pytestmark = pytest.mark.gpu

ACCEPT = 9.21
FIELDS = ("cand", "nis", "logdet", "min_nis", "all_nis", "all_logdet")


def same_query(a, ka, b, kb, what):
    for name in FIELDS:
        x, y = np.ascontiguousarray(getattr(a, name)[ka]), np.ascontiguousarray(getattr(b, name)[kb])
        assert rm.bits_equal(x, y), f"{what}: {name} differs in {int((x.view(np.uint8) != y.view(np.uint8)).reshape(x.size, -1).any(axis=1).sum()) if x.shape == y.shape else -1} entries"


# ---- 1: the query against the single filter, bit for bit ---------------------------------------------------------------------------
def query_against_slots(sd, f, N, m, rng):
    """Three hypotheses stepped twice with labelled observations (dense rows), adopted into slots 1..3: each slot's associate
    against the bank's row."""
    K = 3
    with f.hypotheses(K) as bank:
        for i in range(2):
            obs = [hs.observe(f.mean(0), [(7 * k + 5 * i + 3 * j) % N for j in range(3)], rng) for k in range(K)]
            bank.step([0.004, 0.006, 0.002], [0.02, 0.01, 0.03], [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
        rows = np.stack([bank.rows(k) for k in range(K)])
        assert (np.abs(rows[:, :, 3:]).max(axis=(1, 2)) > 0).all(), "a hypothesis has no cross terms"
        _, zr, zb = hs.observe(f.mean(0), rng.choice(N, m, replace=False), rng)
        got = bank.associate(zr, zb, full=True)
        assert got.cand.shape == (K, m, 2) and got.all_nis.shape == (K, m, N) and (got.cand[:, :, 0] >= 0).all()
        for k in range(K):
            bank.adopt(k, f, k + 1)
        ref = f.associate(np.broadcast_to(zr, (K + 1, m)).copy(), np.broadcast_to(zb, (K + 1, m)).copy(), full=True)
        for k in range(K):
            same_query(got, k, ref, k + 1, f"N = {N}, hypothesis {k} against slot {k + 1}")
        # hypotheses differ, so must their scores
        assert not rm.bits_equal(got.all_nis[0], got.all_nis[1])


def test_query_equals_the_single_filter_s_on_adopted_slots(sd, both_paths):
    with hs.mapped_handle(sd, 4, 20) as f:
        query_against_slots(sd, f, 20, 5, np.random.default_rng(3))
        assert path_ran(f, both_paths)


@pytest.mark.parametrize("N", [70, 130])
def test_query_equals_the_single_filter_s_across_chunk_edges(sd, N):
    with hs.mapped_handle(sd, 4, N) as f:
        query_against_slots(sd, f, N, 8, np.random.default_rng(4))
        assert sd.load_library().ekf_debug_small_launches(f._h) == 0


def test_query_equals_the_single_filter_s_in_the_panel_layout(sd):
    N = 2050
    slam = [[10, 2045, 2046, 2047, 2049], [2046, 2047, 11, 2049], [2045, 2046, 10, 0, 1, 2]]
    with hs.sparse_handle(sd, 4, N, slam, 5) as f:
        query_against_slots(sd, f, N, 3, np.random.default_rng(5))


# ---- 2: the query against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, K, m", ham.CASES)
def test_query_against_the_model(sd, N, K, m):
    totals = ham.new_totals()
    with hs.mapped_handle(sd, 1, N) as f:
        mean = f.mean(0)
        with f.hypotheses(K) as bank:
            bank.reset(ham.seeds(mean, N, K), ham.RESET_BLOCK)                 # (hypothesis 0 at the slot's own pose)
            _, zr, zb = ham.observations(mean, N, m)
            got = bank.associate(zr, zb, full=True)
            states = ham.bank_states(f, bank)
            ham.judge(got, states, zr, zb, f.config.meas_sigma, totals, what=f"N = {N}, K = {K}, m = {m}: ")
            print(f"N = {N}, K = {K}, m = {m}: {totals}")
            assert totals["obs"] == K * m and totals["entries"] == K * m * N
            assert totals["excused"] == 0 and totals["left_out"] == 0, totals
            # a hypothesis's result does not depend on K, on k or on which hypotheses share the launch
            for k in sorted({0, 1, K // 2, K - 2, K - 1}):
                same_query(bank.associate(zr, zb, full=True, k=k), 0, got, k, f"hypothesis {k} queried alone")
            part = bank.associate(zr, zb, full=True, k=(1, K - 1))
            same_query(part, K - 2, got, K - 1, "the last hypothesis in a range from 1")
            lean = bank.associate(zr, zb)
            assert lean.all_nis is None and all(rm.bits_equal(getattr(lean, n), getattr(got, n)) for n in FIELDS[:4])


# ---- 3: the guarantee --------------------------------------------------------------------------------------------------------------
GN = 70
TIGHT = np.diag([1e-4] * 3)


def tight_handle(sd, B):
    """A handle of B slots on a SHARP map of GN landmarks (the mapping run starts at a known pose, every landmark is observed,
    noise 0.02 / 0.03): a wrong pose shows in the NIS.  Slot 0 mapped, the others forks of it."""
    world = orc.synthetic_world(GN, 12)
    diag = world[3].copy()
    diag[:3] = 1e-6
    f = sd.EkfSlam(3 + 2 * GN, batch=B, config=sd.EkfConfig(motion_sigma=0.02, meas_sigma=0.03))
    for b in range(B):
        f.set_state_diag(world[2], diag, b)
    rng = np.random.default_rng(7)
    none = [[]] * (B - 1)
    for c in range(0, GN, 14):
        o = hs.observe(f.mean(0), np.arange(c, min(GN, c + 14)), rng)
        f.step(0.004, 0.02, [o[0]] + none, [o[1]] + none, [o[2]] + none)
    f.flush()
    if B > 1:
        f.fork(0)
    return f


def contested_list(mean, m):
    """m observations from the map's pose: landmark `a` of the closest pair and the most isolated landmark `iso` first, m - 4
    others, then `a` and `iso` AGAIN, 0.02 apart in bearing: two contested landmarks -- the loser of `a` has the pair's other
    landmark to fall to, the loser of `iso` has nothing near."""
    xy = mean[3:].reshape(-1, 2)
    d = np.linalg.norm(xy[:, None] - xy[None], axis=2) + 9.0 * np.eye(GN)
    a, b = (int(v) for v in np.unravel_index(d.argmin(), d.shape))
    iso = int(np.argmax(d.min(axis=1)))
    rng = np.random.default_rng(5)
    others = [int(l) for l in rng.permutation(GN) if l not in (a, b, iso)][:m - 4]
    lms, zr, zb = hs.observe(mean, np.array([a, iso] + others), rng, 0.01)
    return (a, b, iso), np.concatenate([zr, zr[:2]]), np.concatenate([zb, zb[:2] + 0.02])


def engineer(bank, mean, K):
    """Seeds on the first landmark's circle, then: 0 at the map's pose, sharp; 1 at the map's pose, vague (everything finds a
    candidate); 2 ten metres away, sharp (nothing does); 3 a tenth of a metre off, sharp (accepted, but with a NIS the gate refuses)."""
    bank.reset(ham.seeds(mean, GN, K), ham.RESET_BLOCK)
    bank.reset(mean[:3], TIGHT, 0)
    bank.reset(mean[:3], np.diag([0.3 ** 2] * 3), 1)
    bank.reset(mean[:3] + [10.0, 0.0, 0.0], TIGHT, 2)
    bank.reset(mean[:3] + [0.1, 0.0, 0.0], TIGHT, 3)


def host_route(bank, lin, ang, zr, zb, pred=True):
    """The guarantee's sequence; returns the host's assignment and the bank behind the prediction."""
    if pred:
        bank.step(lin, ang, [], [], [])
    mid = hs.snapshot(bank)
    res = bank.associate(zr, zb)
    idx, rr, bb, assign = ham.host_lists(res, zr, zb, ACCEPT)
    bank.update(idx, rr, bb)
    return assign, mid, res


@pytest.mark.parametrize("K, per", [(8, False), (8, True), (65, False), (65, True)])
def test_step_unlabelled_keeps_the_guarantee(sd, K, per):
    rng = np.random.default_rng(K + per)
    lin = 0.004 + 0.002 * rng.random(K) if per else 0.004
    ang = 0.02 + 0.01 * rng.random(K) if per else 0.02
    with tight_handle(sd, 1) as f, f.hypotheses(K) as dev, f.hypotheses(K) as host:
        mean = f.mean(0)
        for bank in (dev, host):
            engineer(bank, mean, K)
            bank.set_nis_gate(threshold=1.5)
        assert hs.same_snapshot(hs.snapshot(dev), hs.snapshot(host))
        (a, b, iso), zr, zb = contested_list(mean, 9)
        m = len(zr)
        # ---- step A: m = 9, both contested outcomes, all accepted, all dropped, an accepted observation the gate rejects ----
        dev.step_unlabelled(lin, ang, zr, zb, accept=ACCEPT)
        want, mid, res = host_route(host, lin, ang, zr, zb)
        got, after = dev.assignments(), hs.snapshot(dev)
        assert got.shape == (K, m) and np.array_equal(got, want), f"assignments differ for hypotheses {np.flatnonzero((got != want).any(axis=1))}"
        assert ham.judge_assignment(got, res, ACCEPT) is None
        assert hs.same_snapshot(after, hs.snapshot(host)), "step_unlabelled is not the host sequence bit for bit"
        print(f"K = {K}, per-hypothesis motion {per}: accepted per hypothesis {list((got >= 0).sum(axis=1))[:8]} ..., rejected by the gate {list(after.n_rej[:8])}")
        # the contested landmarks, in hypothesis 0: the earlier sighting keeps `a` and `iso`; the loser of `a` falls to the pair's
        # other landmark and is accepted, the loser of `iso` is dropped
        assert {got[0, 0], got[0, m - 2]} == {a, b} and {got[0, 1], got[0, m - 1]} == {iso, -1}, got[0]
        assert res.cand[0, 0, 0] == res.cand[0, m - 2, 0] and res.cand[0, 1, 0] == res.cand[0, m - 1, 0] == iso
        assert (got[0, 2:m - 2] >= 0).all()
        assert (got[1] >= 0).all(), f"hypothesis 1 does not accept everything: {got[1]}"
        assert (got[2] == -1).all(), f"hypothesis 2 does not drop everything: {got[2]}"
        for name in ("pose", "blk", "rows", "loglik", "n_obs", "n_rej", "flags"):     # ... and is the prediction-only step
            assert rm.bits_equal(getattr(after, name)[2], getattr(mid, name)[2]), f"hypothesis 2, all dropped: {name} moved"
        assert after.n_obs[2] == 0 and after.n_obs[0] == m - 1 and after.n_obs[1] == m
        assert (got[3] >= 0).any() and after.n_rej[3] >= 1, "hypothesis 3: no accepted observation was rejected by the gate"
        assert np.array_equal(after.n_obs, (got >= 0).sum(axis=1)), "n_obs counts what the update sees"
        # ---- step B: m = 16 ----
        _, zr, zb = contested_list(np.concatenate([hs.snapshot(dev).pose[0], mean[3:]]), 16)
        dev.step_unlabelled(lin, ang, zr, zb, accept=ACCEPT)
        want, _, res = host_route(host, lin, ang, zr, zb)
        got = dev.assignments()
        assert got.shape == (K, 16) and np.array_equal(got, want) and ham.judge_assignment(got, res, ACCEPT) is None
        assert hs.same_snapshot(hs.snapshot(dev), hs.snapshot(host)), "m = 16"
        assert (got[0] >= 0).sum() >= 14 and (got[2] == -1).all()
        # ---- step C: m = 0 is the prediction alone ----
        dev.step_unlabelled(lin, ang, [], [])
        host.step(lin, ang, [], [], [])
        assert dev.assignments().shape == (K, 0) and hs.same_snapshot(hs.snapshot(dev), hs.snapshot(host)), "m = 0"
        # ---- update_unlabelled behind a step with m = 0 ----
        (_, _, _), zr, zb = contested_list(mean, 9)
        dev.step_unlabelled(lin, ang, zr, zb)
        host.step(lin, ang, [], [], [])
        host.update_unlabelled(zr, zb)
        assert np.array_equal(dev.assignments(), host.assignments())
        assert hs.same_snapshot(hs.snapshot(dev), hs.snapshot(host)), "update_unlabelled behind step(m = 0)"


# ---- 4: miss ---------------------------------------------------------------------------------------------------------------------
def test_miss_adds_the_clutter_term_and_nothing_else(sd):
    K, miss = 8, -7.5
    with tight_handle(sd, 1) as f, f.hypotheses(K) as zero, f.hypotheses(K) as pen, f.hypotheses(K) as pred:
        mean = f.mean(0)
        for bank in (zero, pen, pred):
            engineer(bank, mean, K)
            obs = hs.observe(mean, [3, 40, 66])                           # log-likelihoods that are not zero; hypothesis 1 stays vague
            bank.update(*[[o if k != 1 else o[:0] for k in range(K)] for o in obs])
        _, zr, zb = contested_list(mean, 9)
        pred.step(0.004, 0.02, [], [], [])
        zero.step_unlabelled(0.004, 0.02, zr, zb, miss=0.0)
        pen.step_unlabelled(0.004, 0.02, zr, zb, miss=miss)
        L0, a, b = hs.snapshot(pred).loglik, hs.snapshot(zero), hs.snapshot(pen)
        assert np.array_equal(zero.assignments(), pen.assignments())
        dropped = (pen.assignments() < 0).sum(axis=1)
        assert dropped.max() == len(zr) and dropped.min() == 0 and 0 < dropped[0] < len(zr)
        for name in ("pose", "blk", "rows", "n_obs", "n_rej", "flags"):
            assert rm.bits_equal(getattr(a, name), getattr(b, name)), f"miss moved {name}"
        ll = a.loglik - L0                                                 # what the miss = 0 run added
        want = (L0 + dropped * miss) + ll
        ulp = np.spacing(np.maximum.reduce([np.abs(L0), np.abs(dropped * miss), np.abs(ll), np.abs(want)]))
        gap = np.abs(b.loglik - want)
        print(f"miss = {miss}: dropped {list(dropped)}, largest gap {np.max(gap / ulp):.2f} ulp of the largest term (bar 4)")
        assert (gap <= 4.0 * ulp).all()
        assert rm.bits_equal(b.loglik[dropped == 0], a.loglik[dropped == 0]), "nothing dropped: loglik must not be written"
        assert rm.bits_equal(b.loglik[2], L0[2] + len(zr) * miss), "all dropped: one product, one addition"


# ---- 5: what the launches leave alone ------------------------------------------------------------------------------------------------
def test_scoring_writes_nothing_it_should_not(sd):
    K = 5
    with tight_handle(sd, 3) as f, f.hypotheses(K) as bank:
        mean = f.mean(0)
        engineer(bank, mean, K)
        bank.step(0.004, 0.02, *hs.observe(mean, [1, 2, 50]))
        bank.adopt(0, f, 1)
        before, slot, frozen = hs.snapshot(bank), f.state(1), hs.frozen_part(sd, f, 1)
        _, zr, zb = contested_list(mean, 16)
        bank.associate(zr, zb, full=True)
        bank.associate(zr, zb, k=(2, 3))
        assert hs.same_snapshot(hs.snapshot(bank), before), "associate changed the bank"
        assert hs.frozen_same(hs.frozen_part(sd, f, 1), frozen) and np.array_equal(f.state(1)[0], slot[0]) and np.array_equal(f.state(1)[1], slot[1])
        with pytest.raises(sd.EkfError, match="no unlabelled step"):
            bank.assignments()
        bank.step_unlabelled(0.004, 0.02, zr, zb, miss=-3.0)
        bank.adopt(1, f, 2)                                                # succeeds: the map copy is bit for bit the untouched fork's
        hs.assert_same_bits(bank, 1, f, 2, "adopted behind an unlabelled step")


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_bank_alone(sd):
    K = 4
    lib = sd.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    with tight_handle(sd, 1) as f, f.hypotheses(K) as bank:
        engineer(bank, f.mean(0), K)
        before = hs.snapshot(bank)
        zr, zb = np.array([1.0, 0.5]), np.array([0.1, -0.2])
        cand, out = np.zeros((K, 2, 2), dtype=np.int32), np.zeros((K, 2, GN))
        z = lambda a: a.ctypes.data_as(dp)
        assoc = lambda k0, cnt, r, b, m, c, an, al, cap: lib.ekf_hypotheses_associate(bank._h, k0, cnt, r, b, m, c, None, None, None, an, al, cap)
        ci = cand.ctypes.data_as(ip)
        for call, why in ((lambda: assoc(-1, 1, z(zr), z(zb), 2, ci, None, None, 0), b"range outside"),
                          (lambda: assoc(1, K, z(zr), z(zb), 2, ci, None, None, 0), b"range outside"),
                          (lambda: assoc(0, K, z(zr), z(zb), -1, ci, None, None, 0), b"m must lie"),
                          (lambda: assoc(0, K, z(zr), z(zb), 17, ci, None, None, 0), b"m must lie"),
                          (lambda: assoc(0, K, z(np.array([1.0, np.nan])), z(zb), 2, ci, None, None, 0), b"non-finite"),
                          (lambda: assoc(0, K, z(zr), z(np.array([np.inf, 0.0])), 2, ci, None, None, 0), b"non-finite"),
                          (lambda: assoc(0, K, z(zr), z(zb), 2, None, None, None, 0), b"NULL cand"),
                          (lambda: assoc(0, K, z(zr), z(zb), 2, ci, z(out), None, GN), b"together"),
                          (lambda: assoc(0, K, z(zr), z(zb), 2, ci, None, z(out), GN), b"together"),
                          (lambda: assoc(0, K, z(zr), z(zb), 2, ci, z(out), z(out), GN - 1), b"cap is below")):
            assert call() == -1 and why in lib.ekf_hyp_last_error(bank._h), why
        for kw, why in ((dict(lin=np.nan), "non-finite lin"), (dict(ang=np.inf), "non-finite lin"), (dict(accept=-1.0), "accept must be"),
                        (dict(accept=np.nan), "accept must be"), (dict(miss=np.inf), "miss must be finite"), (dict(miss=np.nan), "miss must be finite"),
                        (dict(ranges=[1.0, np.nan]), "non-finite observation"), (dict(bearings=[-np.inf, 0.0]), "non-finite observation")):
            args = dict(lin=0.004, ang=0.02, ranges=zr, bearings=zb, accept=ACCEPT, miss=0.0)
            args.update(kw)
            with pytest.raises(sd.EkfError, match=why):
                bank.step_unlabelled(**args)
            if "lin" not in kw and "ang" not in kw:
                args.pop("lin"), args.pop("ang")
                with pytest.raises(sd.EkfError, match=why):
                    bank.update_unlabelled(**args)
        assert lib.ekf_hypotheses_update_unlabelled(bank._h, z(zr), z(zb), 17, ACCEPT, 0.0) == -1
        assert lib.ekf_hypotheses_step_unlabelled(bank._h, z(zr), z(zb), 2, z(zr), z(zb), 2, ACCEPT, 0.0) == -1
        with pytest.raises(sd.EkfError, match="no unlabelled step"):
            bank.assignments()
        assert lib.ekf_hypotheses_download_assignment(bank._h, 0, K, None) == -1
        assert hs.same_snapshot(hs.snapshot(bank), before)
        bank.step_unlabelled(0.004, 0.02, zr, zb)                          # and the bank still steps
        assert bank.assignments().shape == (K, 2)


# ---- 7: the kidnapped robot without ids ------------------------------------------------------------------------------------------------
def test_kidnapped_robot_without_ids(sd):
    """hypotheses_model's world: 64 seeds on the circle of one sighting, 25 steps of four unlabelled observations each with
    resample_if(0.5, split = 0.3) behind every step.  With the clutter term the winner is the truth; without it a hypothesis that
    matches nothing is never penalised (printed, not asserted)."""
    from slam_duckietown_amd import evaluation as ev
    from slam_duckietown_amd import frontend
    world, mean0, diag0, lin, ang, idx, zr, zb, m = hm.slam_stream()
    steps = 25
    with sd.EkfSlam(3 + 2 * hm.N, batch=2, config=sd.EkfConfig(motion_sigma=hm.MOTION_SIGMA, meas_sigma=hm.MEAS_SIGMA)) as f:
        for b in range(2):
            f.set_state_diag(mean0, diag0, b)
        f.stream_upload(*(np.repeat(x, 2, 1) for x in (lin, ang, idx, zr, zb, m)))
        f.stream_run(0, hm.SLAM_STEPS)
        f.flush()
        f.fork(0)
        mean = f.mean(0)
        rng = np.random.default_rng(77)
        zr0, zb0 = hm.sight(hm.TRUE_POSE, world[hm.SIGHTED], rng, hm.OBS_NOISE)
        seeds = frontend.poses_on_circle(mean[3 + 2 * hm.SIGHTED:5 + 2 * hm.SIGHTED], zr0[0], zb0[0], hm.K)
        cfg = hm.model_cfg()
        pose, run = hm.TRUE_POSE.copy(), []
        for k in range(steps):
            pose, _ = orc.motion_model(pose, 0.004, 0.02, cfg)
            vis = (4 * k + np.arange(hm.M) * 5) % hm.N
            run.append(hm.sight(pose, world[vis], rng, hm.OBS_NOISE))
        for miss in (ev.clutter_loglik(ACCEPT, hm.MEAS_SIGMA), 0.0):
            with f.hypotheses(hm.K) as bank:
                bank.reset(seeds, hm.SEED_COV)
                draws = np.random.default_rng(3)
                for r, b in run:
                    bank.step_unlabelled(0.004, 0.02, r, b, accept=ACCEPT, miss=miss)
                    bank.resample_if(0.5, split=0.3, rng=draws)
                won = ev.resolve_hypotheses(bank)
                got = bank.poses()[0][won.best]
                err = got - pose
                ok = np.hypot(err[0], err[1]) < 0.1 and abs(hm.wrap(err[2])) < 0.1
                print(f"kidnapped robot without ids, miss = {miss:.3f}: winner {won.best} (weight {won.weight:.3f}) {np.hypot(err[0], err[1]):.4f} m, "
                      f"{abs(hm.wrap(err[2])):.4f} rad from the truth: {'found' if ok else 'LOST'}")
                if miss != 0.0:
                    assert ok, "the bank did not find the robot"
                    bank.adopt(won.best, f, 1)
                    assert np.array_equal(f.mean(1)[:3], got)
