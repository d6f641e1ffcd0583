"""The table of tests/test_gpu_sequence_bank.py and tests/test_sequence_bank_cpu.py: the ordered pairs of tests/sequence_cases.py
in an UNEVEN BANK, call A on one slot and call B on another.

tests/sequence_cases.py judges the handle's bookkeeping through every ordered pair of calls on ONE trajectory in a handle of
batch 1.  Much of that bookkeeping is bank-wide or a loop over the bank -- bank_n_hi() sizes every step, cadence and small-state
launch by the LARGEST slot; push_floor() re-uploads every slot's floor and returns early while the one `sizes_dirty` flag is up;
pending_k is one counter per handle, so a call that names slot 2 flushes every slot; front_run() rewrites neff_enq of all B
slots; the removal, the direct / linear / transform calls and the queries take a slot or a range; copy and join take index lists
and may read one slot of a bank while writing another; an uploaded stream carries one bound per step AND slot -- and at B = 1
none of it can be wrong.  Here: three slots under n_max = 79,

    slot 0   acts        sequence_cases.start() as it is: 30 landmarks, 26 observed             n = 63   tags 100 ..
    slot 1   bystander   22 landmarks, 18 observed                                              n = 47   tags 140 ..
    slot 2   acts        34 landmarks, 28 observed: already past the 64-column tile edge        n = 71   tags 180 ..

each with its own synthetic_stream seed.  Prelude: the 28 stream steps and three single steps of sequence_cases, for the whole
bank (ranks pending in every slot on the general kernels).  Then operation A on one acting slot, operation B on the OTHER, and a
continuation -- a step and a 4-step stream with real observations for every slot -- whose pass reads whatever A and B left in
every slot.  Case (a, b): A targets slot 0 and B slot 2 when a + b is even, else A slot 2 and B slot 0: every operation is first
and second on both slots.  Each slot sees at most ONE operation, so slot 2 grows to at most 37 landmarks (join) and the largest
state changes hands inside the table: join on slot 0 gives 69 where remove_landmarks on slot 2 gives 67, copy_from gives 27.

OPERATIONS: the 21 functions of sequence_cases.OPS verbatim, plus two that B = 1 cannot hold:

    fork          the target becomes a twin of slot 1 (EkfSlam.fork: copy_from inside one handle);
    join(slot)    the target appends slot 1's map (EkfSlam.join with `other` the handle itself): slot 1 is only read, with ranks
                  pending.  Slot 1 brings 22 landmarks and n_max = 79 holds 38: NO acting slot has room for them (30 + 22, 34 +
                  22), and the join refuses a state above n_max.  So the operation is three calls, as active_bound off/on and
                  the localisation operations are several: remove_landmarks of the target's landmarks 16 .. (16 stay: 16 + 22 =
                  38, n = 79 = n_max exactly), one step of the whole bank that sees landmark 0 and `tail_mid` in every slot (the
                  removal flushed: this makes ranks pending again, in slot 1 too), then the join.

BANK-WIDE CALLS.  step, run_stream, step_detections, the three localisation calls, localize_detections (and the active_bound
option) take the whole bank; the two hypothesis operations make their bank on the TARGET slot and adopt into it: targeted calls,
held to the bystander rule.  The operation's own inputs go to the TARGET; every other slot gets an IDLE input: the same increments, and observations
of landmark 0 and `tail_mid` of its own map, consistent with its own model mean -- informed landmarks far below its bound, so
that an idle slot's own call never raises a bound that A should have raised.  BankDriver makes this expansion ONCE, from the
float64 model's state, and hands every sink (the model, the model in longdouble, the filter) the same float64 arguments.

THE BYSTANDER RULE (assert_bystander), for every slot a targeted call does not name: its mean after the call is its mean before,
bit for bit; its covariance is within PATH_TOL of what it was (ranks pending may have been applied, nothing else: the bound the
project holds between a query with ranks pending and the flushed state); and where nothing was pending for that slot before the
call -- the stored P_base[0, 0] equal to the covariance's, bit for bit -- its stored P_base is np.array_equal to what it was.
No call of the table is excused from it.

Generator keys of its own: [SEED, a, b, 3] for the operations, [SEED, a, b, 4] for the idle detection windows' jitter."""
import functools

import numpy as np

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import fuzz_model as fz
from tests import linear_model as lm
from tests import parity_blocks as pb
from tests import sequence_cases as sc
from tests import sequence_model as sm
from tests.streams import stream_from

# slot -> (observed, landmarks, synthetic_stream seed, first tag id); slot 0 is sequence_cases.start().
# Slot 2's seed: 22 came first, and its world is not admissible -- with update_direct on slot 2 the float64 model is up to
# 1.8e-11 (cross) and 5.7e-11 (corr_max) from itself in longdouble, above FLOOR_TOL and ENTRY_FLOOR, in 20 cases; so is seed 23's.
# Seed 24's is: 6.7e-12 and 3.3e-11 over all 400 cases (tests/test_sequence_bank_cpu.py holds it; profiles/sequence_bank.txt).
SLOTS = ((sc.N_OBSERVED, sc.N_LANDMARKS, sc.SEED, sc.TAG0), (18, 22, 21, 140), (28, 34, 24, 180))
B = len(SLOTS)
ACTING, BYSTANDER = (0, 2), 1
CAPACITY = (sc.N_MAX - 3) // 2                             # 38 landmarks
PATH_TOL = 1e-11        # pending ranks applied in another order: a query with ranks pending against the flushed state
#                         (tests/test_gpu_queries_after_calls.py, test_gpu_joint, test_gpu_marginals hold the same figure)
EPS_V = 32 * np.finfo(float).eps * sc.INIT_VAR


@functools.lru_cache(maxsize=None)
def starts():
    """Per slot (mean0, diag0, lin, ang, idx, zr, zb): sequence_cases.start's construction at the slot's own size and seed."""
    out = [sc.start()]
    for n_obs, n_lm, seed, _ in SLOTS[1:]:
        s = orc.synthetic_stream(n_obs, sc.STREAM_STEPS + sc.SINGLE_STEPS, 4, seed)
        rng = np.random.default_rng(300 + seed)
        extra = 2 * (n_lm - n_obs)
        out.append((np.concatenate([s[0], rng.uniform(-1.0, 1.0, extra)]), np.concatenate([s[1], np.full(extra, sc.INIT_VAR)]))
                   + tuple(s[2:]))
    return tuple(out)


def new_model(dtype=np.float64):
    return sm.bank([(s[0], s[1]) for s in starts()], None, sc.sources(), dtype)


def targets(a, b):
    """(the slot A names, the slot B names)."""
    return (0, 2) if (a + b) % 2 == 0 else (2, 0)


# ---- the driver ---------------------------------------------------------------------------------------------------------------
HANDLE_WIDE = ("set_option",)


class BankDriver:
    """sequence_cases.Driver for a bank: hands every call to the model and to the sinks beside it, the TARGETED calls as they
    come (every sink acts on its `target` slot), the calls that take the whole bank expanded to one entry per slot -- the
    target's as the operation gave them, an idle input for every other slot.  `observer(when, name, slot)` is called before
    and after every call ("before" / "after"; slot None: the call names the whole bank)."""

    def __init__(self, model, *sinks, observer=None):
        self.model, self.sinks = model, (model,) + sinks
        self.calls = []                                    # (name, slot or None)
        self.observer = observer or (lambda when, name, slot: None)
        self.rng, self.k = np.random.default_rng(0), 0

    def retarget(self, slot):
        for s in self.sinks:
            s.target = int(slot)

    def send(self, name, targeted, *args, **kw):
        slot = self.model.target if targeted else None
        self.calls.append((name, slot))
        self.observer("before", name, slot)
        for s in self.sinks:
            getattr(s, name)(*args, **kw)
        self.observer("after", name, slot)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *args, **kw: self.send(name, not (name.startswith("bank_") or name in HANDLE_WIDE), *args, **kw)

    # -- idle inputs ----------------------------------------------------------------------------------------------------------
    def idle_obs(self, tr, at=None):
        """Landmark 0 and `tail_mid` of `tr`'s map, seen from `at` (default: its mean), lm.follow_up_obs's offsets."""
        idx = [0, sc.tail_mid(tr)]
        self.k += 1
        zr, zb = lm.follow_up_obs(tr.mean if at is None else at, idx, self.k % 50)
        return idx, zr, zb

    def idle_window(self, tr):
        """A detection window of the tags of landmark 0 and `tail_mid` (those in front of the gate; none is legal)."""
        tag_of = {j: t for t, j in tr.tags.items()}
        ids = [tag_of[j] for j in (0, sc.tail_mid(tr)) if j in tag_of]
        return fz.window_of(self.rng, tr, ids, {}, 2)

    def per_slot(self, mine, idle):
        return [mine if b == self.model.target else idle(tr) for b, tr in enumerate(self.model.t)]

    def bank_of_stream(self, lin, ang, idx, zr, zb):
        """The target's stream (lin, ang [K]; idx, zr, zb [K, m]) as a bank's: [K, B] and [K, B, stride] with m [K, B]; an idle
        slot sees its two landmarks from where the increments take its own model pose."""
        K, mt = np.shape(idx)
        stride = max(mt, 2)
        n = len(self.model.t)
        L, A = np.repeat(np.asarray(lin, dtype=float)[:, None], n, 1), np.repeat(np.asarray(ang, dtype=float)[:, None], n, 1)
        I, M = np.zeros((K, n, stride), dtype=np.int32), np.zeros((K, n), dtype=np.int32)
        R, Z = np.zeros((K, n, stride)), np.zeros((K, n, stride))
        for b, tr in enumerate(self.model.t):
            if b == self.model.target:
                I[:, b, :mt], R[:, b, :mt], Z[:, b, :mt], M[:, b] = idx, zr, zb, mt
                continue
            at = tr.mean.copy()
            for k in range(K):
                at[:3] = orc.motion_model(at[:3], L[k, b], A[k, b], orc.EkfConfig())[0]
                I[k, b, :2], R[k, b, :2], Z[k, b, :2] = self.idle_obs(tr, at)
                M[k, b] = 2
        return L, A, I, R, Z, M

    # -- the bank-wide calls, under the names the operations use -----------------------------------------------------------------
    def step1(self, lin, ang, idx, zr, zb):
        n = len(self.model.t)
        obs = self.per_slot(([int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb]), self.idle_obs)
        self.send("bank_step", False, [lin] * n, [ang] * n, obs)

    def run_stream(self, lin, ang, idx, zr, zb):
        self.send("bank_stream", False, *self.bank_of_stream(lin, ang, idx, zr, zb))

    def step_detections(self, lin, ang, win):
        n = len(self.model.t)
        self.send("bank_detections", False, [lin] * n, [ang] * n, self.per_slot(win, self.idle_window))

    def localize1(self, lin, ang, idx, zr, zb):
        n = len(self.model.t)
        obs = self.per_slot(([int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb]), self.idle_obs)
        self.send("bank_localize", False, [lin] * n, [ang] * n, obs, True)

    def localize_update1(self, idx, zr, zb):
        n = len(self.model.t)
        obs = self.per_slot(([int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb]), self.idle_obs)
        self.send("bank_localize", False, [0.0] * n, [0.0] * n, obs, False)

    def run_localize_stream(self, lin, ang, idx, zr, zb):
        self.send("bank_localize_stream", False, *self.bank_of_stream(lin, ang, idx, zr, zb))

    def localize_detections(self, lin, ang, win, unmatched):
        """(an idle window holds tags of the slot's own table only: nothing of it may come back unmatched)"""
        n = len(self.model.t)
        self.send("bank_localize_detections", False, [lin] * n, [ang] * n, self.per_slot(win, self.idle_window),
                  self.per_slot(list(unmatched), lambda tr: []))


# ---- the two operations only a bank can hold -----------------------------------------------------------------------------------
def op_fork(drv, rng):
    drv.fork(BYSTANDER, drv.model.target)


def op_join_slot(drv, rng):
    """Room for slot 1's map, ranks pending again in every slot, then the join (module docstring)."""
    tr = drv.model.tr
    room = CAPACITY - drv.model.t[BYSTANDER].n_lm
    assert 13 <= room < tr.n_lm                            # (`tail_mid` = 12 stays, and stays informed)
    drv.remove_landmarks(list(range(room, tr.n_lm)))
    sc.observe(drv, rng, [0, sc.tail_mid(drv.model.tr)])
    drv.join_slot(BYSTANDER)


# (fork and join(slot) keep the indices 18 and 19 they had: the 400 older cases keep their slots, ids and draws; the three
# operations sequence_cases gained since follow them)
SHARED_BEFORE = 18
OPS = sc.OPS[:SHARED_BEFORE] + (("fork", op_fork), ("join(slot)", op_join_slot)) + sc.OPS[SHARED_BEFORE:]
PAIRS = [(a, b) for a in range(len(OPS)) for b in range(len(OPS))]
TARGETED = ("set_state_diag", "set_tag_index", "predict_linear", "predict_dense1", "update_direct", "update_linear", "transform",
            "join", "join_slot", "fork", "remove_landmarks", "add_landmarks", "copy_in", "hyp_adopt", "hyp_resample_adopt")


def pair_name(a, b):
    ta, tb = targets(a, b)
    return f"{OPS[a][0]} on {ta} then {OPS[b][0]} on {tb}"


def pair_id(a, b):
    return pair_name(a, b).replace(" ", "_").replace("/", "-")


def setup(drv):
    drv.set_option("active_bound", 1)
    for b, (s, (_, n_lm, _, tag0)) in enumerate(zip(starts(), SLOTS)):
        drv.retarget(b)
        drv.set_state_diag(s[0], s[1])
        drv.set_tag_index({tag0 + j: j for j in range(n_lm)})
    drv.retarget(0)


def prelude(drv):
    """sequence_cases.prelude for the whole bank: every slot runs its own stream (m = 4 everywhere)."""
    ss = starts()
    k = sc.STREAM_STEPS
    lin, ang = (np.stack([s[i][:k] for s in ss], 1) for i in (2, 3))
    idx, zr, zb = (np.stack([s[i][:k] for s in ss], 1) for i in (4, 5, 6))
    drv.bank_stream(lin, ang, idx, zr, zb, np.full((k, B), idx.shape[2], dtype=np.int32))
    for k in range(sc.STREAM_STEPS, sc.STREAM_STEPS + sc.SINGLE_STEPS):
        drv.bank_step([s[2][k] for s in ss], [s[3][k] for s in ss],
                      [([int(i) for i in s[4][k]], [float(x) for x in s[5][k]], [float(x) for x in s[6][k]]) for s in ss])


def continuation(drv, rng):
    """sequence_cases.continuation with REAL observations for every slot: a step that names landmark 0, a loose landmark and the
    last one of each map, then a 4-step stream over each map's landmarks in turn."""
    obs = []
    for tr in drv.model.t:
        _, never, last = sc.pick(tr)
        idx = list(dict.fromkeys([0, never, last]))
        zr, zb = lm.follow_up_obs(tr.mean, idx, int(rng.integers(0, 50)))
        obs.append((idx, zr, zb))
    drv.bank_step([0.004] * B, [0.02] * B, obs)
    st = [stream_from(tr.mean, 4, 3, int(rng.integers(1 << 30))) for tr in drv.model.t]
    lin, ang, idx, zr, zb = (np.stack([s[i] for s in st], 1) for i in range(5))
    drv.bank_stream(lin, ang, idx, zr, zb, np.full((4, B), 3, dtype=np.int32))


def run_case(drv, a, b, judge=None):
    """setup, prelude, A on its slot, B on the other, the continuation; `judge(stage)` after the prelude ("start": ranks are
    pending), after A, after B and after the continuation ("A", "B", "end")."""
    rng = np.random.default_rng([sc.SEED, a, b, 3])
    drv.rng, drv.k = np.random.default_rng([sc.SEED, a, b, 4]), 0
    judge = judge or (lambda stage: None)
    ta, tb = targets(a, b)
    setup(drv)
    prelude(drv)
    judge("start")
    drv.retarget(ta)
    OPS[a][1](drv, rng)
    judge("A")
    drv.retarget(tb)
    OPS[b][1](drv, rng)
    judge("B")
    continuation(drv, rng)
    judge("end")


# ---- a front that raises one slot's bound over the 64-column tile edge ---------------------------------------------------------
# front_run() hands the covariance pass its grid through neff_enq, for ALL slots, and the grid counts 64-column tiles.  Behind
# the prelude every slot's bound lies below column 64 (55, 39, 59), and the operations of the table name the FIRST loose landmark:
# slot 2's bound goes to 61, in the same tile -- a slot whose neff_enq the front forgot costs nothing there (the device mutant of
# profiles/sequence_bank.txt passes all 400 pairs).  Here a linear and a direct update of slot 2 name landmark 31: the bound
# becomes 67, one tile further than any slot had, and the pass behind the front must cover it.
EDGE_LANDMARK, EDGE_SLOT = 31, 2


def op_linear_edge(drv, rng):
    tr = drv.model.tr
    a, far = sc.pick(tr)[0], EDGE_LANDMARK
    offset = tr.mean[3 + 2 * far:5 + 2 * far] - tr.mean[3 + 2 * a:5 + 2 * a] + np.array([0.1, -0.2])
    drv.update_linear(*lm.constraint_rows(a, far, offset, np.eye(2) * 0.05 ** 2))


def op_direct_edge(drv, rng):
    """sequence_cases.op_update_direct with the loose landmark at the edge, then the constraint: the direct fix alone leaves
    the landmark's cross terms exact zeros, and the bound where it was."""
    tr = drv.model.tr
    a, far = sc.pick(tr)[0], EDGE_LANDMARK + 1
    z, R = dm.make_fixes(rng, tr.mean, tr.cov, [dm.POSE, a])
    sig = rng.uniform(0.3, 0.6, 2)
    Rn, zn = np.zeros((3, 3)), np.zeros(3)
    Rn[:2, :2] = np.diag(sig ** 2)
    zn[:2] = tr.mean[3 + 2 * far:5 + 2 * far] + np.sqrt(0.01 + sig ** 2) * rng.normal(size=2)
    drv.update_direct([dm.POSE, a, far], z + [zn], R + [Rn])
    op_linear_edge(drv, rng)


EDGE_OPS = (("update_linear", op_linear_edge), ("update_direct, update_linear", op_direct_edge))


def run_edge_case(drv, i, judge=None):
    """setup, prelude, EDGE_OPS[i] on slot 2, the continuation; `judge` after the prelude, the operation and the continuation
    ("start", "A", "end")."""
    rng = np.random.default_rng([sc.SEED, i, 5])
    drv.rng, drv.k = np.random.default_rng([sc.SEED, i, 6]), 0
    judge = judge or (lambda stage: None)
    setup(drv)
    prelude(drv)
    judge("start")
    drv.retarget(EDGE_SLOT)
    EDGE_OPS[i][1](drv, rng)
    judge("A")
    continuation(drv, rng)
    judge("end")


def as_got(model, b):
    """Slot b of a model as a `got` (sequence_cases.as_got)."""
    mean, cov, tags = model.state(b)
    cov = np.asarray(cov, dtype=float)
    return np.asarray(mean, dtype=float), (cov + cov.T) / 2, tags, 0


# ---- the bystander rule --------------------------------------------------------------------------------------------------------
def assert_bystander(before, after, what=""):
    """`before`, `after`: (mean, covariance, stored P_base[0, 0], stored P_base) of a slot that a targeted call did not name,
    read around the call without a download.  -> whether nothing was pending before the call (and P_base was compared)."""
    (m0, P0, raw0, base0), (m1, P1, _, base1) = before, after
    assert np.shape(m1) == np.shape(m0) and np.shape(P1) == np.shape(P0), f"{what}size: {np.shape(m0)} became {np.shape(m1)}"
    bad = np.flatnonzero(np.asarray(m1) != np.asarray(m0))
    assert not len(bad), f"{what}mean: {len(bad)} entries moved (first at {bad[0]}: {m0[bad[0]]!r} -> {m1[bad[0]]!r})"
    err = pb.state_errors((m1, P1), (m0, P0), sc.INIT_VAR)
    whole = orc.rel_fro(P1, P0)
    lim = {"pose": PATH_TOL, "cross": PATH_TOL, "landmarks": PATH_TOL, "corr_max": pb.PATH_CORR_TOL}
    bad = [f"{p}: {err[p]:.3e} exceeds {v:g}" for p, v in lim.items() if p in err and not err[p] < v]
    assert not bad and whole < PATH_TOL, f"{what}covariance moved beyond what applying pending ranks explains: whole {whole:.3e}; " + "; ".join(bad)
    assert err.get("loose_zeros", 0) == 0 and err.get("loose_block", 0.0) <= EPS_V, f"{what}loose landmarks moved: {err}"
    idle = raw0 == P0[0, 0]
    if idle:
        diff = np.flatnonzero(np.asarray(base1) != np.asarray(base0)) if np.shape(base1) == np.shape(base0) else [-1]
        assert not len(diff), f"{what}P_base: nothing was pending, and {len(diff)} stored doubles changed (first at {diff[0]})"
    return bool(idle)
