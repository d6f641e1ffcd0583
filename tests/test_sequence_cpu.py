"""CPU: what makes tests/test_gpu_sequence_pairs.py a statement about device code (no GPU).

Admissibility: every one of the 225 ordered pairs of tests/sequence_cases.py is run on the dense model twice -- in float64, as
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


def test_all_225_pairs_are_admissible(floors):
    assert len(floors) == 225 == len(sc.OPS) ** 2 and all(set(s) == {"start", "A", "B", "end"} for s in floors.values())
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
    assert len(s[0]) == 63 and sc.N_MAX == 79 and len(sc.OPS) == 15 and len(set(n for n, _ in sc.OPS)) == 15
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
                     "set_state_diag", "set_tag_index"}
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
