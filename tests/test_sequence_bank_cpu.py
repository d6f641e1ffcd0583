"""CPU: what makes tests/test_gpu_sequence_bank.py a statement about device code (no GPU).

Admissibility: every one of the 529 cases of tests/sequence_bank_cases.py is run on the dense bank model twice -- in float64, as
the GPU test runs it, and in longdouble (tests/sequence_model.py: the same code, 64 bits of mantissa) -- and every SLOT is judged
after A, after B and after the continuation under sequence_cases' own constants: every relative-Frobenius piece at most
FLOOR_TOL, every entrywise piece at most ENTRY_FLOOR (a tenth of ENTRY_TOL).  No case is excused; one set of draws was chosen for
it, slot 2's world (sequence_bank_cases.SLOTS has the reason).

The table is what it promises: sizes, growth, the largest state changing hands, every operation in both positions on both slots.

The judge is not blind to what only a bank can get wrong: a targeted call applied to the slot beside the one named, a removal
that lowers ANOTHER slot's bound, a bank-wide step sized by the smallest slot -- each fails in a named case, by name; and the
bystander rule fails for one ulp in one entry."""
import numpy as np
import pytest

from tests import parity_blocks as pb
from tests import sequence_bank_cases as bc
from tests import sequence_cases as sc
from tests import sequence_model as sm

FROBENIUS = ("pose", "cross", "landmarks", "mean_pose")
ENTRYWISE = ("corr_max", "mean_landmarks", "loose_cross")
NAMES = [n for n, _ in bc.OPS]


@pytest.fixture(scope="module")
def runs():
    """(a, b) -> ({stage: [per slot {piece: float64 model against longdouble model}]}, {stage: [landmarks per slot]}, calls)."""
    assert np.finfo(np.longdouble).eps < 1e-18, "longdouble is no wider than float64 here: the comparison would say nothing"
    out = {}
    for a, b in bc.PAIRS:
        m64, mld = bc.new_model(np.float64), bc.new_model(np.longdouble)
        stages, sizes = {}, {}

        def judge(stage):
            errs = []
            for s in range(bc.B):
                t64, tld = m64.t[s], mld.t[s]
                assert tld.cov.dtype == np.longdouble and t64.cov.dtype == np.float64
                assert len(t64.mean) == len(tld.mean) and t64.tags == tld.tags and np.array_equal(t64.seen, tld.seen)
                errs.append(pb.state_errors(bc.as_got(m64, s)[:2], mld.state(s)[:2], sc.INIT_VAR))
            stages[stage], sizes[stage] = errs, [tr.n_lm for tr in m64.t]

        d = bc.BankDriver(m64, mld)
        bc.run_case(d, a, b, judge)
        out[a, b] = (stages, sizes, d.calls)
    return out


def pieces(runs, names):
    """(value, case, stage, slot, piece) of every measured piece in `names`."""
    return [(e[p], bc.pair_name(a, b), st, s, p) for (a, b), (stages, _, _) in runs.items() for st, errs in stages.items()
            for s, e in enumerate(errs) for p in names if p in e]


def test_all_cases_are_admissible(runs):
    assert len(runs) == 529 == len(bc.OPS) ** 2 and all(set(r[0]) == {"start", "A", "B", "end"} for r in runs.values())
    for pos, name in ((0, "first"), (1, "second")):
        for i, op in enumerate(NAMES):
            for slot in range(bc.B):
                w = {p: max((e[slot][p] for ab, (stages, _, _) in runs.items() if ab[pos] == i for e in stages.values() if p in e[slot]),
                            default=0.0) for p in pb.STATE_PIECES}
                print(f"FLOOR {op:20s} {name:6s} slot {slot} {pb.fmt_state(w)}")
    w = max(pieces(runs, FROBENIUS))
    print(f"FLOOR worst relative-Frobenius piece: {w[4]} = {w[0]:.2e} ({w[1]}, after {w[2]}, slot {w[3]}); FLOOR_TOL = {sc.FLOOR_TOL:g}")
    bad = [x for x in pieces(runs, FROBENIUS) if not x[0] <= sc.FLOOR_TOL]
    assert not bad, f"the model in float64 and in longdouble differ by more than {sc.FLOOR_TOL:g}: the case needs other inputs: {bad[:5]}"
    for (a, b), (stages, _, _) in runs.items():
        for st, errs in stages.items():
            for s, e in enumerate(errs):
                what = (bc.pair_name(a, b), st, s, e)
                assert e.get("loose_zeros", 0) == 0, what
                assert e.get("loose_block", 0.0) <= bc.EPS_V / 4 and e.get("loose_mean", 0.0) <= sc.FLOOR_TOL, what


def test_the_entrywise_floor_stays_under_the_shared_constant(runs):
    """ENTRY_TOL is sequence_cases' constant, unchanged: ten times ENTRY_FLOOR, which bounds the worst entrywise piece of all
    529 bank cases too (fork and join(slot) included; profiles/sequence_bank.txt has the figures)."""
    w = max(pieces(runs, ENTRYWISE))
    print(f"FLOOR worst entrywise piece: {w[4]} = {w[0]:.2e} ({w[1]}, after {w[2]}, slot {w[3]}); ENTRY_FLOOR = {sc.ENTRY_FLOOR:g}")
    for op in ("fork", "join(slot)"):
        i = NAMES.index(op)
        v = max(x for x in pieces({ab: r for ab, r in runs.items() if i in ab}, ENTRYWISE))
        print(f"FLOOR worst entrywise piece with {op}: {v[4]} = {v[0]:.2e} ({v[1]}, after {v[2]}, slot {v[3]})")
    assert sc.ENTRY_TOL == 10 * sc.ENTRY_FLOOR and w[0] <= sc.ENTRY_FLOOR, w


def test_the_table_is_what_it_promises(runs):
    ss = bc.starts()
    assert [len(s[0]) for s in ss] == [63, 47, 71] and sc.N_MAX == 79 and len(bc.OPS) == 23 and len(set(NAMES)) == 23
    assert bc.OPS[:18] == sc.OPS[:18] and NAMES[18:20] == ["fork", "join(slot)"] and bc.OPS[20:] == sc.OPS[18:] and len(sc.OPS) == 21
    tags = [set(range(t0, t0 + n)) for _, n, _, t0 in bc.SLOTS]
    assert not (tags[0] & tags[1] or tags[1] & tags[2] or tags[0] & tags[2]) and len({s for _, _, s, _ in bc.SLOTS}) == 3
    for s, (n_obs, _, _, _) in zip(ss, bc.SLOTS):
        assert set(np.unique(s[4][:sc.STREAM_STEPS + sc.SINGLE_STEPS])) == set(range(n_obs))
    # the start behind the prelude: informed and loose landmarks where the table says, exact zeros beyond
    m = bc.new_model()
    d = bc.BankDriver(m)
    bc.setup(d)
    bc.prelude(d)
    for tr, (n_obs, n_lm, _, t0) in zip(m.t, bc.SLOTS):
        loose, informed = pb.loose_landmarks(tr.cov, sc.INIT_VAR)
        assert loose.tolist() == list(range(n_obs, n_lm)) and len(informed) == n_obs and tr.tags == {t0 + j: j for j in range(n_lm)}
        assert not tr.cov[3 + 2 * n_obs:, :3 + 2 * n_obs].any() and tr.seen.tolist() == [True] * n_obs + [False] * (n_lm - n_obs)
        assert sc.tail_mid(tr) == 12 < n_obs                # (an idle slot's two landmarks are informed, far below its bound)
    # sizes: nothing outgrows the handle, in ANY case; the figures of the table
    for (a, b), (_, sizes, _) in runs.items():
        assert max(max(s) for s in sizes.values()) <= bc.CAPACITY, (bc.pair_name(a, b), sizes)
        assert all(s[bc.BYSTANDER] == 22 for s in sizes.values()), (bc.pair_name(a, b), sizes)
    join, remove, copy, jslot, fork = (NAMES.index(x) for x in ("join", "remove_landmarks", "copy_from", "join(slot)", "fork"))
    assert bc.targets(join, remove) == (0, 2) and runs[join, remove][1]["B"] == [33, 22, 32]      # n = 69 and 67: slot 0 leads
    assert bc.targets(remove, join) == (0, 2) and runs[remove, join][1]["B"] == [28, 22, 37]
    assert runs[copy, copy][1]["B"] == [12, 22, 12] and runs[jslot, jslot][1]["end"] == [38, 22, 38]
    assert bc.targets(fork, join) == (2, 0) and runs[fork, join][1]["B"] == [33, 22, 22] and max(s[2] for r in runs.values() for s in r[1].values()) == 38
    hands = [ab for ab, (_, sizes, _) in runs.items() if int(np.argmax(sizes["B"])) != 2]
    print(f"the largest state is not slot 2's after B in {len(hands)} cases")
    assert (join, remove) in hands and len(hands) > 20
    # every operation first and second on both acting slots; the bystander is never named
    seen = {(x, pos, bc.targets(a, b)[pos]) for a, b in bc.PAIRS for pos, x in enumerate((a, b))}
    assert seen == {(x, pos, s) for x in range(23) for pos in (0, 1) for s in bc.ACTING}
    behind_setup = 1 + 2 * bc.B                              # set_option, then (set_state_diag, set_tag_index) per slot
    for (a, b), (_, _, calls) in runs.items():
        assert all(slot != bc.BYSTANDER for _, slot in calls[behind_setup:]), bc.pair_name(a, b)
        assert {n for n, slot in calls if slot is not None} <= set(bc.TARGETED), calls
    every = set().union(*({n for n, _ in r[2]} for r in runs.values()))
    assert every == set(bc.TARGETED) | {"set_option", "bank_step", "bank_stream", "bank_detections", "bank_localize", "bank_localize_stream",
                                           "bank_localize_detections"}


def test_an_idle_slot_never_raises_its_own_bound():
    """Behind the prelude every idle input names landmarks 0 and 12 only: the bound an idle slot's own call implies, 29, lies
    far below the slot's (39 for the bystander)."""
    m = bc.new_model()
    d = bc.BankDriver(m)
    bc.setup(d)
    bc.prelude(d)
    d.retarget(0)
    for tr in m.t[1:]:
        assert d.idle_obs(tr)[0] == [0, 12] and sc.model_bound(tr) >= 39
    L, A, I, R, Z, M = d.bank_of_stream(*sc.stream_from(m.tr.mean, 3, 4, 1))
    assert M.tolist() == [[4, 2, 2]] * 3 and I[:, 1:, :2].tolist() == [[[0, 12]] * 2] * 3 and (L == 0.004).all()
    w = d.idle_window(m.t[1])
    assert {t.tag_id for _, tags in w for t in tags} <= {140, 152}


@pytest.mark.parametrize("i", range(len(bc.EDGE_OPS)))
def test_the_tile_edge_cases_are_admissible_and_cross_the_edge(i):
    """run_edge_case: behind the prelude every slot's bound lies below column 64; the front on slot 2 takes its bound to 67 (the
    direct fix alone leaves it at 59); float64 against longdouble under the shared constants, every slot, every stage."""
    m64, mld = bc.new_model(np.float64), bc.new_model(np.longdouble)
    bounds = {}

    def judge(stage):
        bounds[stage] = [sc.model_bound(tr) for tr in m64.t]
        for s in range(bc.B):
            e = pb.state_errors(bc.as_got(m64, s)[:2], mld.state(s)[:2], sc.INIT_VAR)
            assert all(e[p] <= sc.FLOOR_TOL for p in FROBENIUS if p in e) and all(e[p] <= sc.ENTRY_FLOOR for p in ENTRYWISE if p in e), (stage, s, e)
            assert e.get("loose_zeros", 0) == 0 and e.get("loose_block", 0.0) <= bc.EPS_V / 4 and e.get("loose_mean", 0.0) <= sc.FLOOR_TOL

    d = bc.BankDriver(m64, mld)
    bc.run_edge_case(d, i, judge)
    assert bounds["start"] == [55, 39, 59] and bounds["A"] == [55, 39, 67] and (67 - 1) // 64 > (59 - 1) // 64
    assert [c for c in d.calls if c[1] is not None][-1] == ("update_linear", 2)
    if "update_direct" in bc.EDGE_OPS[i][0]:
        m = bc.new_model()
        d = bc.BankDriver(m)
        bc.setup(d)
        bc.prelude(d)
        d.retarget(bc.EDGE_SLOT)
        seen = m.tr.seen.copy()
        d.update_linear = lambda *a, **k: None             # (the direct fix alone)
        bc.op_direct_edge(d, np.random.default_rng([sc.SEED, i, 5]))
        assert np.array_equal(m.tr.seen, seen) and sc.model_bound(m.tr) == 59 and m.tr.cov[3 + 2 * 32, 3 + 2 * 32] < 1.0


# ---- the judge is not blind: mutants only a bank can express -------------------------------------------------------------------
PIECE = "(pose|cross|landmarks|corr_max|mean_pose|mean_landmarks|loose_block|loose_mean|loose_cross|size|tags): "


def judged(got, want):
    """(mean, covariance) of one slot against the model's, under the GPU module's judge (tags and flags apart)."""
    return pb.assert_state_close((got[0], (got[1] + got[1].T) / 2, {}, 0), (want[0], want[1], {}), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL)


def case(first, second):
    return NAMES.index(first), NAMES.index(second)


def test_a_targeted_call_applied_to_the_slot_beside_is_caught():
    """Mutant a, in "transform(cov) on 0 then step on 2": transform(b = 0) lands on slot 1.  Slot 0 (not moved) and slot 1 (moved)
    both fail after A; slot 2 passes."""
    class Beside(sm.SeqBank):
        def transform(self, T, cov=None):
            self.target += 1
            sm.SeqBank.transform(self, T, cov)
            self.target -= 1

    a, b = case("transform(cov)", "step")
    assert bc.targets(a, b) == (0, 2)
    m, bad = bc.new_model(), Beside([(s[0], s[1]) for s in bc.starts()], None, sc.sources())
    failed = {}

    def judge(stage):
        for s in range(bc.B):
            try:
                judged(bc.as_got(bad, s)[:2], m.state(s)[:2])
            except AssertionError as e:
                failed.setdefault(stage, {})[s] = str(e)

    bc.run_case(bc.BankDriver(m, bad), a, b, judge)
    print("MUTANT a", failed.get("A"))
    assert "start" not in failed and set(failed["A"]) == {0, 1} and not any(2 in v for v in failed.values())
    assert all("mean_landmarks" in v or "mean_pose" in v for v in failed["A"].values())


def test_a_removal_that_lowers_another_slots_bound_is_caught():
    """Mutant b, in "remove_landmarks on 2 then step on 0": the removal of two landmarks from slot 2 takes their four columns off
    slot 1's bound as well (39 -> 35).  Slot 1's next pass is B's step, in which it is idle -- its own bound is 29 --: rows and
    columns 35 .. stay what they were before the step."""
    a, b = case("remove_landmarks", "step")
    assert bc.targets(a, b) == (2, 0)
    m = bc.new_model()
    kept = {}

    def judge(stage):
        kept[stage] = (m.t[1].mean.copy(), m.t[1].cov.copy(), sc.model_bound(m.t[1]))

    d = bc.BankDriver(m)
    bc.run_case(d, a, b, judge)
    assert [c for c in d.calls if c[0] == "remove_landmarks"] == [("remove_landmarks", 2)]
    before, after = kept["A"], kept["B"]
    assert before[2] == after[2] == 39 and np.array_equal(kept["start"][1], before[1])     # (the removal left slot 1 alone)
    judged(after, after)
    for bound, caught in ((39, False), (35, True)):
        got = sc.keep_rows_beyond(before, after, bound)
        if not caught:
            judged(got, after)
            continue
        with pytest.raises(AssertionError, match="(cross|landmarks|corr_max): .* exceeds") as why:
            judged(got, after)
        print("MUTANT b", why.value)


def test_a_step_sized_by_the_smallest_slot_is_caught():
    """Mutant c, in "step on 0 then step on 2": B's step runs every slot as if it had the smallest slot's size, 47 -- the columns
    beyond stay what they were.  Slot 1 (the smallest) is right; slots 0 and 2, whose step names their LAST landmark, are not."""
    a, b = case("step", "step")
    assert bc.targets(a, b) == (0, 2)
    m = bc.new_model()
    kept = {}

    def judge(stage):
        kept[stage] = [(tr.mean.copy(), tr.cov.copy()) for tr in m.t]

    bc.run_case(bc.BankDriver(m), a, b, judge)
    n_lo = min(len(s[0]) for s in kept["A"])
    assert n_lo == 47
    for s in range(bc.B):
        got = sc.keep_rows_beyond(kept["A"][s], kept["B"][s], n_lo)
        if s == 1:
            judged(got, kept["B"][s])
            continue
        with pytest.raises(AssertionError, match=PIECE) as why:
            judged(got, kept["B"][s])
        print(f"MUTANT c slot {s}", why.value)


def test_the_bystander_rule_sees_one_ulp():
    m = bc.new_model()
    d = bc.BankDriver(m)
    bc.setup(d)
    bc.prelude(d)
    mean, cov, _, _ = bc.as_got(m, 1)
    base = np.triu(cov).ravel()                            # (a stand-in for the stored triangle)
    idle, pending = (mean, cov, cov[0, 0], base), (mean, cov, cov[0, 0] * 0.9, base)
    assert bc.assert_bystander(idle, (mean.copy(), cov.copy(), cov[0, 0], base.copy())) is True
    up = lambda x: np.nextafter(x, np.inf)
    moved = mean.copy()
    moved[7] = up(moved[7])
    with pytest.raises(AssertionError, match="mean: 1 entries moved"):
        bc.assert_bystander(pending, (moved, cov, cov[0, 0], base))
    stored = base.copy()
    stored[5] = up(stored[5])
    with pytest.raises(AssertionError, match="P_base: nothing was pending, and 1 stored doubles changed"):
        bc.assert_bystander(idle, (mean, cov, cov[0, 0], stored))
    # ranks were pending: the stored matrix may move, the covariance by no more than their application explains
    assert bc.assert_bystander(pending, (mean, cov, cov[0, 0], stored)) is False
    P = cov.copy()
    P[3, 0] = P[0, 3] = P[0, 3] + 1e-9 * np.sqrt(P[0, 0] * P[3, 3])
    with pytest.raises(AssertionError, match="covariance moved beyond"):
        bc.assert_bystander(pending, (mean, P, cov[0, 0], base))
    r = 3 + 2 * 20                                         # a loose landmark of slot 1: an exact zero must stay one
    P = cov.copy()
    P[r, 0] = P[0, r] = 1e-300
    with pytest.raises(AssertionError, match="loose landmarks moved"):
        bc.assert_bystander(pending, (mean, P, cov[0, 0], base))
