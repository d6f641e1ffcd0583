"""CPU: what makes tests/test_gpu_sequence_pairs.py a statement about device code (no GPU).

Admissibility: every one of the 441 ordered pairs of tests/sequence_cases.py is run on the dense model twice -- in float64, as
the GPU test runs it, and in longdouble (tests/sequence_model.py: the same code, 64 bits of mantissa) -- and judged after A,
after B and after the continuation.  Every relative-Frobenius piece of that comparison is at most FLOOR_TOL = 1e-11 (the rule
of tests/test_update_blocks_cpu.py), so TOL = 1e-9 on the GPU is two decades above what the inputs' conditioning explains;
ENTRY_TOL is ten times the worst entrywise piece measured here.  No case is excused.

The judge is not blind: a model damaged the way a stale mirror of csrc/ekf_api.hip would damage the filter fails
parity_blocks.assert_state_close, by name."""
import numpy as np
import pytest

from tests import parity_blocks as pb
from tests import sequence_cases as sc
from tests import sequence_model as sm

FROBENIUS = ("pose", "cross", "landmarks", "mean_pose")
ENTRYWISE = ("corr_max", "mean_landmarks", "loose_cross")
EPS_V = 32 * np.finfo(float).eps * sc.INIT_VAR


@pytest.fixture(scope="module")
def floors():
    """(a, b) -> {stage: {piece: float64 model against longdouble model}}."""
    assert np.finfo(np.longdouble).eps < 1e-18, "longdouble is no wider than float64 here: the comparison would say nothing"
    out = {}
    for a, b in sc.PAIRS:
        m64, mld = sc.new_model(np.float64), sc.new_model(np.longdouble)
        stages = {}

        def judge(stage):
            assert mld.tr.cov.dtype == np.longdouble and m64.tr.cov.dtype == np.float64
            assert len(m64.tr.mean) == len(mld.tr.mean) and m64.tr.tags == mld.tr.tags
            assert np.array_equal(m64.tr.seen, mld.tr.seen)
            stages[stage] = pb.state_errors(sc.as_got(m64)[:2], mld.state()[:2], sc.INIT_VAR)

        sc.run_case(sc.Driver(m64, mld), a, b, judge)
        out[a, b] = stages
    return out


def worst(floors, pieces):
    return max((e[p], sc.pair_name(a, b), st, p) for (a, b), stages in floors.items()
               for st, e in stages.items() for p in pieces if p in e)


def test_all_pairs_are_admissible(floors):
    assert len(floors) == 441 == len(sc.OPS) ** 2 and all(set(s) == {"start", "A", "B", "end"} for s in floors.values())
    for pos, name in ((0, "first"), (1, "second")):
        for i, (op, _) in enumerate(sc.OPS):
            w = {p: max((e[p] for ab, stages in floors.items() if ab[pos] == i for e in stages.values() if p in e), default=0.0)
                 for p in pb.STATE_PIECES}
            print(f"FLOOR {op:20s} {name:6s} {pb.fmt_state(w)}")
    bad = [(sc.pair_name(a, b), st, p, e[p]) for (a, b), stages in floors.items() for st, e in stages.items()
           for p in FROBENIUS if p in e and not e[p] <= sc.FLOOR_TOL]
    assert not bad, f"the model in float64 and in longdouble differ by more than {sc.FLOOR_TOL:g}: the case needs other inputs: {bad[:5]}"
    for (a, b), stages in floors.items():
        for st, e in stages.items():
            what = (sc.pair_name(a, b), st, e)
            assert e.get("loose_zeros", 0) == 0, what
            # (the reference's own rounding takes at most a quarter of what the judge allows a loose landmark's own block)
            assert e.get("loose_block", 0.0) <= EPS_V / 4 and e.get("loose_mean", 0.0) <= sc.FLOOR_TOL, what


def test_entry_tol_is_ten_times_the_measured_floor(floors):
    w = worst(floors, ENTRYWISE)
    print(f"FLOOR worst entrywise piece: {w[3]} = {w[0]:.2e} ({w[1]}, after {w[2]}); ENTRY_TOL = {sc.ENTRY_TOL:g}")
    assert sc.ENTRY_TOL == 10 * sc.ENTRY_FLOOR and sc.ENTRY_TOL < pb.REL_TOL
    assert sc.ENTRY_FLOOR / 3 <= w[0] <= sc.ENTRY_FLOOR, w   # (a rounding-level quantity moves with the BLAS's order of summation)


def test_the_table_is_what_it_promises():
    s = sc.start()
    assert len(s[0]) == 63 and sc.N_MAX == 79 and len(sc.OPS) == 21 and len(set(n for n, _ in sc.OPS)) == 21
    assert set(np.unique(s[4][:sc.STREAM_STEPS + sc.SINGLE_STEPS])) == set(range(sc.N_OBSERVED))
    sizes, calls = {}, {}
    for a, b in sc.PAIRS:
        if a == b or a == 0 or b == 0:
            m = sc.new_model()
            d = sc.Driver(m)
            sc.run_case(d, a, b)
            sizes[a, b], calls[a, b] = m.tr.n_lm, d.calls
    assert max(sizes.values()) <= 38 and sizes[9, 9] == 36 and sizes[12, 12] == 34 and sizes[2, 2] == 32
    every = set().union(*calls.values())
    assert every >= {"step1", "run_stream", "step_detections", "predict_linear", "predict_dense1", "update_direct",
                     "update_linear", "transform", "join", "remove_landmarks", "add_landmarks", "copy_in", "set_option",
                     "set_state_diag", "set_tag_index", "localize1", "localize_update1", "run_localize_stream",
                     "localize_detections", "hyp_adopt", "hyp_resample_adopt"}
    assert [n for n, _ in sc.OPS[15:]] == list(sc.LOCALIZE_OPS) and len(sc.LOCALIZE_OPS) == 6    # appended: the older pairs keep their ids and draws
    assert [n for n, _ in sc.OPS[15:18]] == ["localize", "localize_update", "run_localize"]
    # the start: 26 informed landmarks, 4 loose ones with exact zeros; growth crosses the 64-column edge
    m = sc.new_model()
    d = sc.Driver(m)
    sc.setup(d)
    sc.prelude(d)
    loose, informed = pb.loose_landmarks(m.tr.cov, sc.INIT_VAR)
    assert loose.tolist() == [26, 27, 28, 29] and len(informed) == 26 and len(m.tr.mean) == 63
    assert not m.tr.cov[3 + 2 * 26:, :3 + 2 * 26].any() and m.tr.seen.tolist() == [True] * 26 + [False] * 4


# ---- the judge is not blind --------------------------------------------------------------------------------------------------
def reference(ops):
    m = sc.new_model()
    d = sc.Driver(m)
    sc.setup(d)
    sc.prelude(d)
    rng = np.random.default_rng(5)
    for op in ops:
        op(d, rng)
    return m, d, rng


def judged(got, model, entry_tol=sc.ENTRY_TOL):
    return pb.assert_state_close((got[0], (got[1] + got[1].T) / 2, model.tr.tags, 0), model.state(), sc.INIT_VAR, sc.TOL, entry_tol)


def test_a_bound_one_landmark_too_low_is_caught():
    m, d, rng = reference([])
    before = (m.tr.mean.copy(), m.tr.cov.copy())
    sc.observe(d, rng, [0, 25])                            # the highest informed landmark: the bound must cover it
    judged(m.state(), m)
    got = sc.keep_rows_beyond(before, m.state(), 3 + 2 * 25)
    with pytest.raises(AssertionError, match="landmarks: .* exceeds|corr_max: .* exceeds"):
        judged(got, m)


def test_a_removed_landmarks_column_left_in_place_is_caught():
    m, d, rng = reference([])
    before = (m.tr.mean.copy(), m.tr.cov.copy())
    sc.op_remove(d, rng)
    a, never, _ = 0, 26, None
    assert len(m.tr.mean) == 59
    judged(m.state(), m)
    rows = np.delete(np.arange(63), [3 + 2 * a, 4 + 2 * a, 3 + 2 * never, 4 + 2 * never])
    cols = np.delete(np.arange(63), [3 + 2 * 29, 4 + 2 * 29, 3 + 2 * never, 4 + 2 * never])   # landmark a's column stays, the last goes
    up = np.triu(before[1][np.ix_(rows, cols)])            # (the device keeps the upper triangle)
    got = (before[0][rows], up + np.triu(up, 1).T)
    assert np.array_equal(np.delete(np.delete(before[1], np.setdiff1d(np.arange(63), rows), 0), np.setdiff1d(np.arange(63), rows), 1),
                          m.tr.cov)
    with pytest.raises(AssertionError, match="(cross|landmarks|corr_max): .* exceeds"):
        judged(got, m)


def test_a_bound_that_did_not_rise_after_a_transform_with_a_covariance_is_caught():
    m, d, rng = reference([sc.op_transform_cov])
    before = (m.tr.mean.copy(), m.tr.cov.copy())
    assert m.tr.seen.all() and before[1][3 + 2 * 26:, :3].any()     # the loose landmarks are correlated now
    sc.observe(d, rng, [0, 3])
    err = judged(m.state(), m)
    assert err["loose_cross"] < 1e-15 and len(pb.loose_landmarks(m.tr.cov, sc.INIT_VAR)[0]) == 4
    got = sc.keep_rows_beyond(before, m.state(), 3 + 2 * 26)         # the bound of before the transform
    with pytest.raises(AssertionError, match="loose_cross|loose_mean"):
        judged(got, m)


# ---- localisation: no pass repairs a pose-row column that a call skipped -------------------------------------------------------
START_BOUND = 3 + 2 * sc.N_OBSERVED                        # the bound of the start after its prelude: 55
PIECE = "(pose|cross|landmarks|corr_max|mean_pose|mean_landmarks|loose_block|loose_mean|loose_cross): "


def stale_bound_bank():
    """A model whose localisation leaves P(0..2, c) and its mirror as they were for every c at or beyond max(the start's
    bound, the call's own bound): what k_loc_rows does when the operation before it did not raise the bound it trusts -- and
    k_hyp_rows, when ekf_hyp_create took a bound from before A for the bank (planted mistake a)."""
    def stale(call, named):
        def wrapped(self, *args, **kw):
            tr = self.tr
            was = tr.cov.copy()
            call(self, *args, **kw)
            c = max(START_BOUND, 3 + 2 * (max(int(j) for j in named(tr, *args)) + 1))
            tr.cov[:3, c:], tr.cov[c:, :3] = was[:3, c:], was[c:, :3]
        return wrapped

    def matched(tr, lin, ang, win, unmatched):
        return [tr.tags[t.tag_id] for _, tags in win for t in tags if t.tag_id in tr.tags]

    class StaleBound(sm.SeqBank):
        localize1 = stale(sm.SeqBank.localize1, lambda tr, lin, ang, idx, *rest, **kw: idx)
        localize_detections = stale(sm.SeqBank.localize_detections, matched)

        def hyp_resample_adopt(self, motion, one, two, pose0, cov0, u, s, z):
            """(step one and step two each under their own bound; the split in between keeps 1 - s^2 of every column)"""
            tr = self.tr
            was = (1.0 - s * s) * tr.cov
            mean, cov = self._hyp_resampled(motion[0], one, pose0, cov0, u, s, z)
            for obs, step in ((one, None), (two, motion[1])):
                if step is not None:
                    was = cov
                    mean, cov = sm.lcm.literal_step(mean, cov, *step, *obs, tr.cfg)
                c = max(START_BOUND, 3 + 2 * (max(int(j) for j in obs[0]) + 1))
                cov[:3, c:], cov[c:, :3] = was[:3, c:], was[c:, :3]
            tr.mean, tr.cov = mean, cov
            tr.seen[np.asarray(list(one[0]) + list(two[0]), dtype=int)] = True

    s = sc.start()
    return StaleBound(s[0], s[1], sc.sources())


RAISES_THE_BOUND = ("transform(cov)", "predict_dense", "join", "update_linear", "step", "step_detections")


@pytest.mark.parametrize("op", sc.LOCALIZE_OPS)
def test_localisation_under_a_bound_that_A_did_not_raise_is_caught(op):
    """Behind each operation that correlates columns at or beyond the start's bound -- transform(cov) and join among them --,
    for each of the six localisation-like operations (hyp_adopt is two localize1 calls: the mutant's too).  The weakest of the
    first 18 is transform(cov) then localize_update -- no prediction, so the stale columns differ only
    by K_p (H P)[:, c], and c is a loose landmark's: every informed piece passes and loose_cross, measured 1.9e-9,
    stands against ENTRY_TOL = 4e-10, a factor of 5; the next, transform(cov) then localize, has loose_cross at 5.5e-7
    (profiles/localize_pairs.txt)."""
    names = [n for n, _ in sc.OPS]
    for first in RAISES_THE_BOUND:
        m, bad = sc.new_model(), stale_bound_bank()
        d = sc.Driver(m, bad)
        sc.setup(d)
        sc.prelude(d)
        rng = np.random.default_rng([5, names.index(first), names.index(op)])
        sc.OPS[names.index(first)][1](d, rng)
        assert sc.model_bound(m.tr) > START_BOUND and np.array_equal(bad.tr.cov, m.tr.cov), first
        sc.OPS[names.index(op)][1](d, rng)
        judged(sc.as_got(m), m)
        with pytest.raises(AssertionError, match=PIECE) as why:
            judged(sc.as_got(bad), m)
        e = pb.state_errors(sc.as_got(bad)[:2], m.state()[:2], sc.INIT_VAR)
        print(f"MUTANT stale bound  {first:16s} then {op:16s} {pb.fmt_state(e)} | {why.value}")
        if (first, op) == ("transform(cov)", "localize_update"):
            assert "loose_cross" in str(why.value) and max(e[p] for p in pb.PIECES) < sc.TOL


def test_a_pass_that_skips_what_localize_correlated_is_caught():
    """localize names a loose landmark: its pose cross-covariance is non-zero now, and the next SLAM step's pass moves its own
    block too.  A pass with the bound of before the call leaves that block as it was."""
    m, d, rng = reference([sc.op_localize])
    assert sc.model_bound(m.tr) == START_BOUND + 2 and m.tr.cov[:3, START_BOUND:START_BOUND + 2].any()
    before = (m.tr.mean.copy(), m.tr.cov.copy())
    sc.observe(d, rng, [0, 3])
    judged(m.state(), m)
    got = sc.keep_rows_beyond(before, m.state(), START_BOUND)
    with pytest.raises(AssertionError, match="loose_block"):
        judged(got, m)


@pytest.mark.parametrize("op", (sc.op_hyp_adopt, sc.op_hyp_resample_adopt), ids=("hyp_adopt", "hyp_resample_adopt"))
def test_an_adoption_that_leaves_the_bound_where_it_was_is_caught(op):
    """Planted mistake b.  The adopted hypothesis named a loose landmark: the pose rows it brings reach past the slot's bound,
    and ekf_hyp_adopt must raise every mirror.  A pass with the bound of before the adoption -- B = step's, or the
    continuation's -- leaves that landmark's rows as they were."""
    m, d, rng = reference([op])
    assert sc.model_bound(m.tr) == START_BOUND + 2 and m.tr.cov[:3, START_BOUND:START_BOUND + 2].any()
    before = (m.tr.mean.copy(), m.tr.cov.copy())
    sc.op_step(d, rng)
    judged(m.state(), m)
    got = sc.keep_rows_beyond(before, m.state(), START_BOUND)
    with pytest.raises(AssertionError, match="landmarks: .* exceeds") as why:      # (the step observed it: informed now)
        judged(got, m)
    print(f"MUTANT adoption, bound not raised: {why.value}")


@pytest.mark.parametrize("first", ("transform(cov)", "join"))
def test_a_resampling_copy_that_keeps_the_dead_slots_bound_is_caught(first):
    """Planted mistake c.  Hypothesis 0 was reset: its own bound is 3.  k_hyp_copy gives slot 0 the ancestor's rows; with the
    dead slot's bound kept, step two updates the columns below its OWN bound only (it names the first loose landmark) and every
    column beyond -- correlated by A -- stays what the copy brought."""
    class DeadBound(sm.SeqBank):
        def hyp_resample_adopt(self, motion, one, two, *rest):
            tr = self.tr
            mean, cov = self._hyp_resampled(motion[0], one, *rest)
            tr.mean, tr.cov = sm.lcm.literal_step(mean, cov, *motion[1], *two, tr.cfg)
            c = max(3, 3 + 2 * (max(two[0]) + 1))
            tr.cov[:3, c:], tr.cov[c:, :3] = cov[:3, c:], cov[c:, :3]
            tr.seen[np.asarray(list(one[0]) + list(two[0]), dtype=int)] = True

    names = [n for n, _ in sc.OPS]
    s = sc.start()
    m, bad = sc.new_model(), DeadBound(s[0], s[1], sc.sources())
    d = sc.Driver(m, bad)
    sc.setup(d)
    sc.prelude(d)
    rng = np.random.default_rng([6, names.index(first)])
    sc.OPS[names.index(first)][1](d, rng)
    sc.op_hyp_resample_adopt(d, rng)
    judged(sc.as_got(m), m)
    with pytest.raises(AssertionError, match=PIECE) as why:
        judged(sc.as_got(bad), m)
    print(f"MUTANT copy keeps the dead slot's bound, behind {first}: {why.value}")


class LooseTable(sm.SeqBank):
    """localize_detections on a tag table that is not the model's: `wrong(tr, unmatched)` is the table the window meets."""
    wrong = None

    def _localize_window(self, tr, lin, ang, win, unmatched):
        (tr.mean, tr.cov), tags, _ = sm.ldw.model_window(tr.mean, tr.cov, self.wrong(tr, unmatched), win, lin, ang, cfg=tr.cfg)
        tr.seen[np.asarray(list(tags), dtype=int)] = True


def test_localize_detections_matching_the_unknown_tag_is_caught():
    """Planted mistake d, first half: the id the table does not hold is matched all the same (to the tail's landmark)."""
    class Matches(LooseTable):
        wrong = staticmethod(lambda tr, unmatched: {**tr.tags, **{t: sc.tail_mid(tr) for t in unmatched}})

    s = sc.start()
    m, bad = sc.new_model(), Matches(s[0], s[1], sc.sources())
    d = sc.Driver(m, bad)
    sc.setup(d)
    sc.prelude(d)
    sc.op_localize_detections(d, np.random.default_rng(8))
    assert d.calls.count("localize_detections") == 2
    judged(sc.as_got(m), m)
    with pytest.raises(AssertionError, match=PIECE) as why:
        judged(sc.as_got(bad), m)
    print(f"MUTANT the unknown tag matched: {why.value}")


def test_localize_detections_on_a_table_a_removal_left_stale_is_caught():
    """Planted mistake d, second half: behind remove_landmarks the table kept its old numbering -- the tag of the last landmark
    points past the map (the association must not follow it: the window's match is lost) and every other tag one or two
    landmarks too far.  The operation's own two windows, then one that shows the last landmark's tag."""
    class Stale(LooseTable):
        def remove_landmarks(self, lms):
            old = dict(self.tr.tags)
            sm.SeqBank.remove_landmarks(self, lms)
            self.stale = old

        wrong = lambda self, tr, unmatched: self.stale

    s = sc.start()
    m, bad = sc.new_model(), Stale(s[0], s[1], sc.sources())
    d = sc.Driver(m, bad)
    sc.setup(d)
    sc.prelude(d)
    rng = np.random.default_rng(9)
    sc.op_remove(d, rng)
    last = m.tr.n_lm - 1
    assert bad.stale[sc.TAG0 + 29] == 29 > last == m.tr.tags[sc.TAG0 + 29] and np.array_equal(bad.tr.cov, m.tr.cov)
    before = (bad.tr.mean.copy(), bad.tr.cov.copy())
    assert last in sc.tags_in_gate(m.tr)
    d.localize_detections(0.004, 0.02, *sc.detection_window(d, rng, [last]))
    judged(sc.as_got(m), m)
    assert np.array_equal(bad.tr.cov[3:, 3:], before[1][3:, 3:]) and not bad.tr.cov[:3, 3 + 2 * last:].any()    # (nothing matched)
    with pytest.raises(AssertionError, match="loose_cross|pose") as why:
        judged(sc.as_got(bad), m)
    print(f"MUTANT a stale entry past the map: {why.value}")
    sc.op_localize_detections(d, rng)                      # (the other entries: each one or two landmarks off)
    with pytest.raises(AssertionError, match=PIECE):
        judged(sc.as_got(bad), m)


def test_a_landmark_mean_moved_behind_localize_is_caught():
    m, d, rng = reference([sc.op_localize])
    mean, cov, _ = m.state()
    mean = mean.copy()
    mean[3 + 2 * 5] += 1e-7
    with pytest.raises(AssertionError, match="mean_landmarks"):
        judged((mean, cov), m)


def test_the_judge_names_the_whole_state_pieces():
    m, d, rng = reference([sc.op_transform_cov])
    mean, cov, tags = m.state()
    cov = (cov + cov.T) / 2
    ok = lambda **kw: pb.assert_state_close((kw.get("mean", mean), kw.get("cov", cov), kw.get("tags", tags), kw.get("flags", 0)),
                                            (mean, cov, tags), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL)
    assert max(v for k, v in ok().items()) == 0.0 and set(ok()) >= set(pb.STATE_PIECES)
    for piece, kw in (("size", dict(mean=mean[:-2], cov=cov[:-2, :-2])), ("flags", dict(flags=4)),
                      ("tags", dict(tags={t: j for t, j in tags.items() if j})), ):
        with pytest.raises(AssertionError, match=piece):
            ok(**kw)
    r = 3 + 2 * 27

    def edited(i, j, v, sym=True):
        P = cov.copy()
        P[i, j] = v
        if sym:
            P[j, i] = v
        return P

    with pytest.raises(AssertionError, match="asymmetry"):
        ok(cov=edited(1, 7, np.nextafter(cov[1, 7], np.inf), sym=False))
    with pytest.raises(AssertionError, match="loose_block"):
        ok(cov=edited(r, r, cov[r, r] + 2 * EPS_V))
    with pytest.raises(AssertionError, match="loose_cross"):
        ok(cov=edited(r, 0, cov[r, 0] + 2 * sc.ENTRY_TOL * np.sqrt(cov[r, r] * cov[0, 0])))
    with pytest.raises(AssertionError, match="loose_mean"):
        mu = mean.copy()
        mu[r] += 1e-8 * max(1.0, abs(mu[r]))
        ok(mean=mu)
    with pytest.raises(AssertionError, match="pose: .* exceeds"):
        P = cov.copy()
        P[:3, :3] *= 1.0 + 1e-6
        ok(cov=P)
    m0, _, _ = reference([])                               # exact zeros must stay exact zeros
    mean0, cov0, tags0 = m0.state()
    cov0 = (cov0 + cov0.T) / 2
    P = cov0.copy()
    P[r, 0] = P[0, r] = 1e-300
    with pytest.raises(AssertionError, match="loose_cross: 1 entries non-zero"):
        pb.assert_state_close((mean0, P, tags0, 0), (mean0, cov0, tags0), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL)
