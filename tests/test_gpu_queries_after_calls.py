"""GPU: every read-only query behind every state-changing call (tests/sequence_cases.py: run_query_case; the model is
tests/sequence_model.py's, tests/test_queries_after_calls_cpu.py shows that the 21 cases are admissible and the judge not blind).

marginals(), joint() and associate() read the filter "as the covariance pass would leave it" through the mirrors the
state-changing calls maintain: the size word, the mean's current buffer, the pending pose noise, the padded rank count and the
active bound -- an entry takes the pending ranks only below that bound.  The pairs module judges those mirrors through state(),
which flushes; here NOTHING is downloaded until the very end.  Per case: the prelude (ranks pending on the general kernels),
operation A, then a tail of single steps that see landmark 0 and one mid-map landmark -- their own bound lies far below the one A
left, so a query behind them is right only if A's bound reached it.  After A and after the tail, against the dense model:

  joint() over a random permutation of ALL landmarks, permuted back: the whole state, judged by assert_state_close (TOL,
    ENTRY_TOL, exact symmetry, size, tag index, flags), its mean bit-equal to mean();
  joint() of three landmarks (the highest under the bound, a loose one, the tail's): the same bits as that sub-block;
  marginals(): informed blocks and pose at TOL, loose blocks within 32 eps init_var, as many as the model has landmarks;
  associate(full=True) of four observations: assoc_world.check_query against the MODEL's state, none excused, none left out;
  nothing moved: passes, scheduling counters and P_base as they were, every query repeated gives the same bits.

Then, after the tail only: state() -- it flushes -- against the model; the pending-time joint() and marginals() within 1e-11 of
the download (the project's bound for pending ranks summed in another order); the same queries with nothing pending equal to the
download bit for bit; factor() against the downloaded covariance.  On the general kernels ranks must be pending behind the tail
in every case, and behind A at least for predict_linear and step -- and NOT behind a localisation call (localize_detections and the two
hypothesis-bank operations included), which applies what is pending at entry and appends no rank; the small-state path never has any, and its queries before and
after the download agree bit for bit.

Handles are made once per path and reset per case; a failed assertion drops them, a refused or failed call ends the module."""
import time

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import assoc_world as aw
from tests import parity_blocks as pb
from tests import sequence_cases as sc
from tests.conftest import path_ran
from tests.factor_model import check_factor
from tests.gpu_support import pbase, scheduling
from tests.sequence_device import Device

pytestmark = pytest.mark.gpu

PATH_TOL = 1e-11        # a query with ranks pending against the flushed download (test_gpu_joint, test_gpu_marginals)
PATHS = ("default_path", "general_kernels")
BOUND_MUST_RISE = ("step", "step_detections", "predict_dense", "update_linear", "transform(cov)", "join") + sc.LOCALIZE_OPS
PENDING_AT_A = ("predict_linear", "step")
HANDLES = {}            # path -> Device
RECORD = {"cases": set(), "pending": {}, "bounds": {}, "worst": {}, "distance": {}, "seconds": 0.0}
TOTALS = dict.fromkeys(aw.TOTALS, 0)
CASES = list(range(len(sc.OPS)))


@pytest.fixture(scope="module")
def sd():
    import slam_duckietown_amd as sd
    sd.load_library()
    yield sd
    for dev in HANDLES.values():
        dev.close()
    HANDLES.clear()


def device(sd, path):
    if path not in HANDLES:
        HANDLES[path] = Device(sd)
        HANDLES[path].f.profile_enable(True)
    return HANDLES[path]


def same_bits(x, y):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y))


def queries(sd, dev, model, rngs, what):
    """Every query, twice, without a download: judged against the model, and nothing of the filter moved.  -> what was read."""
    f, tr = dev.f, model.tr
    n, N = len(tr.mean), tr.n_lm
    before = (pbase(sd, f, 0), scheduling(sd, f))
    perm = [int(j) for j in rngs[1].permutation(N)]
    sel = sc.query_selection(tr)
    zr, zb = sc.query_obs(rngs[0], tr.mean)

    def read():
        jm, jc = f.joint(perm, 0)
        sm_, scov = f.joint(sel, 0)
        pose, lms = f.marginals(0)
        a = f.associate(zr, zb, full=True)
        return (jm, jc), (sm_, scov), (pose, lms), a

    q = dict(zip(("joint", "joint3", "marginals", "associate"), read()))
    assert f.size() == n, f"{what}size: {f.size()} where the model has {n}"
    mean, cov = sc.unpermute(perm, *q["joint"])
    assert np.array_equal(mean, f.mean()), f"{what}joint: its mean differs from mean()"
    err = pb.assert_state_close((mean, cov, f.tag_index(), f.flags()), model.state(), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL,
                                what=what + "joint: ")
    ix = np.array(sc.sub_idx(sel))
    assert np.array_equal(q["joint3"][1], cov[np.ix_(ix, ix)]) and np.array_equal(q["joint3"][0], mean[ix]), \
        f"{what}joint of landmarks {sel}: not the bits of the whole-map query's sub-block"
    merr = pb.assert_marginal_blocks_close(*q["marginals"], tr.cov, sc.INIT_VAR, sc.TOL, what=what)
    err.update({"marg_" + k: v for k, v in merr.items()})
    assert f.config.meas_sigma == tr.cfg.meas_sigma
    excused = TOTALS["excused"], TOTALS["left_out"]
    aw.check_query(f, lambda b: (tr.mean, tr.cov), zr, zb, what=what + "associate: ", res=q["associate"], totals=TOTALS)
    assert (TOTALS["excused"], TOTALS["left_out"]) == excused, f"{what}associate: an observation excused or an entry left out"
    for name, x, y in zip(q, q.values(), read()):
        assert same_bits(x, y), f"{what}{name}: repeated, it returns other bits"
    assert np.array_equal(pbase(sd, f, 0), before[0]), f"{what}the queries wrote P_base"
    assert scheduling(sd, f) == before[1], f"{what}the queries moved the counters: {before[1]} -> {scheduling(sd, f)}"
    q["state"] = (mean, cov)
    return q, err


@pytest.mark.parametrize("a", CASES, ids=[sc.query_name(a).replace(" ", "_").replace("/", "-") for a in CASES])
def test_queries_after(sd, both_paths, a):
    general = both_paths == "general_kernels"
    dev = device(sd, both_paths)
    f = dev.f
    model = sc.new_model()
    rngs = sc.query_rngs(a)
    name = f"{sc.query_name(a)}, {both_paths}"
    bounds = {}
    t0 = time.perf_counter()

    def pending(tr):
        # ranks pending: the stored P_base[0, 0] is not the covariance's (the pairs module's criterion: the model and the
        # filter agree to 1e-9, one pending single step alone moves the pose variance by far more than 1e-6 of it)
        raw, want = dev.raw00(), float(tr.cov[0, 0])
        return abs(raw - want) > 1e-6 * want

    def judge(stage):
        tr = model.tr
        bounds[stage] = (sc.model_bound(tr), sc.tail_bound(tr), len(tr.mean))
        RECORD["pending"][a, stage, both_paths] = pending(tr)
        if stage == "start":
            return
        what = f"{name}, after {stage}, "
        if general and (stage == "tail" or sc.query_name(a) in PENDING_AT_A):
            assert RECORD["pending"][a, stage, both_paths], f"{what}no ranks pending (P_base[0, 0] = {dev.raw00()})"
        if general and stage == "A" and sc.query_name(a) in sc.LOCALIZE_OPS:
            assert not RECORD["pending"][a, stage, both_paths], f"{what}something is pending (P_base[0, 0] = {dev.raw00()})"
        q, err = queries(sd, dev, model, rngs, what)
        RECORD["worst"][both_paths, a, stage] = err
        if stage != "tail":
            return
        passes = f.profile_passes()
        got = dev.got()                                    # the download: it flushes
        if general:
            assert f.profile_passes() == passes + 1, f"{what}state(): ranks were pending, and the download ran no pass"
        pb.assert_state_close(got, model.state(), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL, what=what + "state(): ")
        mu, P = got[:2]
        assert dev.raw00() == P[0, 0], f"{what}ranks pending behind the download"
        (jmean, jcov), (pose, lms) = q["state"], q["marginals"]
        wpose, wlms = pb.marginal_blocks(P)
        dist = {"joint": orc.rel_fro(jcov, P), "marginals_pose": orc.rel_fro(pose, wpose), "marginals_landmarks": orc.rel_fro(lms, wlms)}
        RECORD["distance"][both_paths, a] = dist
        assert np.array_equal(jmean, mu), f"{what}joint: the pending-time mean is not the download's"
        for piece, d in dist.items():
            assert d < PATH_TOL, f"{what}{piece}: with ranks pending, {d:.3e} from the download exceeds {PATH_TOL:g}"
        # nothing is pending now: the kb == 0 contract of the query kernels, bit for bit
        perm = [int(j) for j in np.random.default_rng([13, a]).permutation(tr.n_lm)]
        now = sc.unpermute(perm, *f.joint(perm, 0))
        assert np.array_equal(now[0], mu) and np.array_equal(now[1], P), f"{what}joint: nothing pending, and not the download's bits"
        npose, nlms = f.marginals(0)
        assert np.array_equal(npose, wpose) and np.array_equal(nlms, wlms), \
            f"{what}marginals: nothing pending, and not the download's bits"
        if not general:                                    # nothing was ever pending there
            assert np.array_equal(jcov, P) and np.array_equal(pose, wpose) and np.array_equal(lms, wlms), \
                f"{what}the small-state path's queries before and after the download differ"
        fac = f.factor(0)
        assert fac.info[0] == 0 and fac.n[0] == len(tr.mean), f"{what}factor(): info {fac.info[0]}, n {fac.n[0]}"
        check_factor(what + "factor()", fac.upper(0), fac.logdet[0], P)
        assert np.array_equal(fac.means[0], mu), f"{what}factor(): its mean is not the download's"
        assert path_ran(f, both_paths), f"{what}not the path {both_paths}"

    try:
        sc.run_query_case(sc.Driver(model, dev), a, judge)
    except AssertionError:
        HANDLES.pop(both_paths).close()
        raise
    except Exception as e:                                 # a call refused or failed: nothing more is started on this device
        HANDLES.pop(both_paths, None)
        pytest.exit(f"{name}: {type(e).__name__}: {e}", returncode=3)
    RECORD["cases"].add((a, both_paths))
    RECORD["bounds"][a] = bounds
    RECORD["seconds"] += time.perf_counter() - t0


def test_the_module_kept_its_promises():
    """Every operation ran on both paths; on the general kernels ranks were pending behind the tail in all 21 cases and behind
    A for predict_linear and step, and nothing behind a localisation A; the bound A left lies above the bound before A and above
    the tail's own for the twelve operations that must raise it; no observation excused, no entry left out.  Prints the worst of
    every piece per operation and stage, and the pending-time queries' distance from the download (profiles/queries_after_calls.txt)."""
    for (path, a, stage), w in sorted(RECORD["worst"].items()):
        print(f"DEVICE {path:15s} {sc.query_name(a):20s} {stage:5s} {pb.fmt_state(w)} | marginals "
              + " ".join(f"{k[5:]}={v:.2e}" for k, v in w.items() if k.startswith("marg_")))
    for (path, a), d in sorted(RECORD["distance"].items()):
        print(f"DISTANCE {path:15s} {sc.query_name(a):20s} " + " ".join(f"{k}={v:.2e}" for k, v in d.items()) + f" (bound {PATH_TOL:g})")
    for a in CASES:
        print(f"PENDING {sc.query_name(a):20s} " + " ".join(
            f"{p}/{st}={RECORD['pending'].get((a, st, p))}" for p in PATHS for st in ("start", "A", "tail")))
    print(f"ASSOCIATE {TOTALS}; {len(RECORD['cases'])} cases in {RECORD['seconds']:.2f} s")
    assert RECORD["cases"] == {(a, p) for a in CASES for p in PATHS}, "not every operation ran on both paths (a selection, or failures)"
    names = [sc.query_name(a) for a in CASES]
    assert all(RECORD["pending"][a, "tail", "general_kernels"] for a in CASES)
    assert all(RECORD["pending"][names.index(op), "A", "general_kernels"] for op in PENDING_AT_A)
    assert not any(RECORD["pending"][names.index(op), "A", "general_kernels"] for op in sc.LOCALIZE_OPS)
    for op in BOUND_MUST_RISE:
        b = RECORD["bounds"][names.index(op)]
        assert b["A"][0] > b["start"][0] and b["A"][0] > b["A"][1] and b["tail"][0] == b["A"][0], (op, b)
    assert TOTALS["obs"] == 2 * len(PATHS) * sc.QUERY_OBS * len(CASES) and TOTALS["excused"] == 0 and TOTALS["left_out"] == 0
