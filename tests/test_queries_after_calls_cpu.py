"""CPU: what makes tests/test_gpu_queries_after_calls.py a statement about device code (no GPU).

Admissibility: each of the 21 cases of sequence_cases.run_query_case (one operation, then a tail of single steps whose own
bound lies mid-map) runs on the dense model in float64 and in longdouble, compared after A and after the tail: every
relative-Frobenius piece at most FLOOR_TOL, every entrywise piece at most ENTRY_FLOOR, a loose landmark's own block within a
quarter of what the judge allows -- the constants of the pairs table, unchanged.  The associate() reference alone excuses no
observation and leaves out no entry for the observations the GPU module draws.

The judge is not blind.  The mutant is a query whose bound is too low: entries at or beyond `bound` keep their value from
before the tail (sequence_cases.keep_rows_beyond).  With the tail steps' own bound it fails the joint judge in all 21 cases
and the marginals judge; with the bound of before A it fails wherever A raised the bound over landmarks the tail's ranks
reach -- at least step, step_detections, predict_dense, update_linear, transform(cov) and join."""
import types

import numpy as np
import pytest

from tests import assoc_world as aw
from tests import parity_blocks as pb
from tests import sequence_cases as sc

FROBENIUS = ("pose", "cross", "landmarks", "mean_pose")
ENTRYWISE = ("corr_max", "mean_landmarks", "loose_cross")
EPS_V = 32 * np.finfo(float).eps * sc.INIT_VAR
BOUND_MUST_RISE = ("step", "step_detections", "predict_dense", "update_linear", "transform(cov)", "join") + sc.LOCALIZE_OPS
# the bound does not rise (or falls: copy_from), or what it newly covers stays uncorrelated with the pose (join(explicit)):
# the second mutant cannot be caught there
BOUND_STAYS = ("run_stream", "predict_linear", "update_direct", "transform", "add_landmarks", "remove_landmarks",
               "join(explicit)", "copy_from")
NAMES = [n for n, _ in sc.OPS]


class ModelQueries:
    """associate() as the reference itself answers it: what aw.check_query excuses or leaves out WITHOUT a device."""
    batch = 1

    def __init__(self, model):
        self.model, self.config = model, model.tr.cfg

    def _unlabelled(self, zr, zb, m):
        return np.asarray(zr)[None, :], np.asarray(zb)[None, :], np.array([len(zr)], dtype=np.int32)

    def associate(self, zr, zb, m=None, full=False):
        mean, cov, _ = self.model.state()
        nis, logdet, _, _ = aw.ref_scores(mean, cov, zr, zb, np.array([self.config.meas_sigma ** 2] * 2))
        cand, cnis, mn, _ = aw.ref_candidates(nis, logdet)
        return types.SimpleNamespace(cand=cand[None], nis=cnis[None], logdet=logdet[cand][None], min_nis=mn[None],
                                     all_nis=nis[None], all_logdet=np.broadcast_to(logdet, nis.shape)[None])


@pytest.fixture(scope="module")
def cases():
    """a -> {stage: what the tests below read}: the float64 model's state, its distance to the longdouble model, the bounds."""
    assert np.finfo(np.longdouble).eps < 1e-18, "longdouble is no wider than float64 here: the comparison would say nothing"
    out, totals, conds = {}, dict.fromkeys(aw.TOTALS, 0), []
    for a in range(len(sc.OPS)):
        m64, mld = sc.new_model(np.float64), sc.new_model(np.longdouble)
        obs_rng, _ = sc.query_rngs(a)
        stages = {}

        def judge(stage):
            tr = m64.tr
            assert mld.tr.cov.dtype == np.longdouble and tr.cov.dtype == np.float64
            assert len(tr.mean) == len(mld.tr.mean) and tr.tags == mld.tr.tags and np.array_equal(tr.seen, mld.tr.seen)
            got = sc.as_got(m64)
            st = stages[stage] = dict(state=(got[0].copy(), got[1].copy()), tags=dict(tr.tags), bound=sc.model_bound(tr),
                                      tail_bound=sc.tail_bound(tr), n=len(tr.mean), sel=sc.query_selection(tr))
            if stage == "start":
                return
            st["err"] = pb.state_errors(got[:2], mld.state()[:2], sc.INIT_VAR)
            st["marg"] = pb.marginal_errors(*pb.marginal_blocks(got[1]), mld.state()[1], sc.INIT_VAR)
            zr, zb = sc.query_obs(obs_rng, tr.mean)
            _, cond = aw.check_query(ModelQueries(m64), lambda b: m64.state()[:2], zr, zb, what=f"{NAMES[a]}, {stage}: ",
                                     totals=totals)
            conds.append(float(cond[0].max()))

        sc.run_query_case(sc.Driver(m64, mld), a, judge)
        out[a] = stages
    out["totals"], out["cond"] = totals, max(conds)
    return out


def judged(got, st, what=""):
    return pb.assert_state_close((got[0], got[1], st["tags"], 0), st["state"] + (st["tags"],), sc.INIT_VAR, sc.TOL,
                                 sc.ENTRY_TOL, what=what)


def mutant(case, bound):
    """The tail's state with every entry at or beyond `bound` as it was before the tail."""
    return sc.keep_rows_beyond(case["A"]["state"], case["tail"]["state"], bound)


def caught(case, bound):
    try:
        judged(mutant(case, bound), case["tail"])
    except AssertionError as e:
        return str(e)
    return None


def test_all_cases_are_admissible(cases):
    for a, name in enumerate(NAMES):
        assert set(cases[a]) == {"start", "A", "tail"}
        for stage in ("A", "tail"):
            e, g = cases[a][stage]["err"], cases[a][stage]["marg"]
            print(f"FLOOR {name:20s} {stage:5s} {pb.fmt_state(e)} | marginals " + " ".join(f"{k}={v:.2e}" for k, v in g.items()))
            what = (name, stage, e, g)
            assert all(e[p] <= sc.FLOOR_TOL for p in FROBENIUS if p in e), what
            assert all(e[p] <= sc.ENTRY_FLOOR for p in ENTRYWISE if p in e), what
            assert e.get("loose_zeros", 0) == 0 and e.get("loose_mean", 0.0) <= sc.FLOOR_TOL, what
            assert e.get("loose_block", 0.0) <= EPS_V / 4 and g.get("loose_block", 0.0) <= EPS_V / 4, what
            assert g["pose"] <= sc.FLOOR_TOL and g["landmarks"] <= sc.FLOOR_TOL, what
            judged(cases[a][stage]["state"], cases[a][stage])          # (the judge passes the model itself)


def test_the_cases_are_what_they_promise(cases):
    """Sizes within the query's 64 landmarks and n_max; the tail sees an informed mid-map landmark below the bound A left; the
    three-landmark selection is three distinct landmarks; where the bound must rise over the tail's reach, it does."""
    for a, name in enumerate(NAMES):
        start, A, tail = (cases[a][s] for s in ("start", "A", "tail"))
        N = (A["n"] - 3) // 2
        assert tail["n"] == A["n"] <= sc.N_MAX and N <= 36 and tail["bound"] == A["bound"] <= A["n"], name
        mid = (A["tail_bound"] - 3) // 2 - 1
        assert mid == min(12, N - 3) and mid in pb.loose_landmarks(A["state"][1], sc.INIT_VAR)[1], name
        assert A["tail_bound"] < A["bound"], name
        for st in (A, tail):
            assert len(st["sel"]) == len(set(st["sel"])) == 3 and all(0 <= l < N for l in st["sel"]), (name, st["sel"])
        print(f"BOUND {name:20s} before A {start['bound']:3d} after A {A['bound']:3d} tail's own {A['tail_bound']:3d} n {A['n']:3d}")
        if name in BOUND_MUST_RISE:
            assert A["bound"] > start["bound"] and A["bound"] > A["tail_bound"], name
    assert cases[NAMES.index("copy_from")]["A"]["n"] == 27 and cases[NAMES.index("copy_from")]["A"]["tail_bound"] == 23


def test_the_reference_alone_excuses_nothing(cases):
    t = cases["totals"]
    print(f"ASSOCIATE reference alone: {t}, worst cond(S) {cases['cond']:.3g}")
    assert t["obs"] == 2 * sc.QUERY_OBS * len(sc.OPS) == 168 and t["entries"] == 4952
    assert t["excused"] == 0 and t["left_out"] == 0


def test_a_query_with_the_tails_own_bound_is_caught_in_all_cases(cases):
    for a, name in enumerate(NAMES):
        why = caught(cases[a], cases[a]["A"]["tail_bound"])
        print(f"MUTANT tail's own bound   {name:20s} {why}")
        assert why is not None, name


def test_a_query_with_the_bound_of_before_A_is_caught_where_A_raised_it(cases):
    """... and demanded only there.  `active_bound off/on` is not demanded either way: the line printed says what happens."""
    for a, name in enumerate(NAMES):
        bound = min(cases[a]["start"]["bound"], cases[a]["A"]["n"])
        why = caught(cases[a], bound)
        print(f"MUTANT bound of before A  {name:20s} ({bound:2d} -> {cases[a]['A']['bound']:2d}) {why}")
        if name in BOUND_MUST_RISE:
            assert why is not None and ("cross" in why or "loose_block" in why or "loose_mean" in why), (name, why)
        else:
            assert name in BOUND_STAYS or name == "active_bound off/on"


def test_marginals_with_the_tails_own_bound_are_caught(cases):
    for a, name in enumerate(NAMES):
        tail = cases[a]["tail"]
        want = tail["state"][1]
        pb.assert_marginal_blocks_close(*pb.marginal_blocks(want), want, sc.INIT_VAR, sc.TOL)
        pose, lms = pb.marginal_blocks(mutant(cases[a], tail["tail_bound"])[1])
        with pytest.raises(AssertionError, match="marginals (landmarks|loose_block)"):
            pb.assert_marginal_blocks_close(pose, lms, want, sc.INIT_VAR, sc.TOL, what=f"{name}: ")
        with pytest.raises(AssertionError, match="marginals count"):
            pb.assert_marginal_blocks_close(pose, lms[:-1], want, sc.INIT_VAR, sc.TOL)
