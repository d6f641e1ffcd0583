"""GPU: ekf_update_linear and ekf_update_direct at every row count, stride and pass form, judged block by block.

k_linear and k_direct are compiled for row caps 4 / 8 / 16 / 32 (36 for direct), chosen by the bank's largest D padded to 4;
the measurement layout depends on the cap and on the call's strides; and both kernels leave state for the covariance pass
behind them (so[b].neff, the zeroed pose noise, the row-slab pass's queue heads).  The cases (tests/update_cases.py; shown
admissible on the CPU by tests/test_update_blocks_cpu.py: the reference's two forms agree on every piece to 1e-11):

  rows     one trajectory, N = 40 on the general kernels, a dense P behind 25 steps: linear D in {1 .. 32} x k in {0 .. 16}
           landmarks in no order, z and innovation mode, a dense correlated R, D > 3 + 2 k included; direct D in {2 .. 33} from a
           pose fix, a position fix or none plus landmarks, some of them never observed.  Every cap edge (4|5, 8|9, 16|17) is hit.
  ragged   banks of 4: (a) a small D inside the largest instantiation with stride > count, (b) cap 8 with one trajectory
           rejected by its gate, (c) one trajectory alone while the others have ranks pending (bit-equal to a flushed twin).
  forms    the pass behind the call: k_flush, k_flush nontemporal, k_flush_rs forced at B = 3 (slabs cut in chunks) and
           B = 8 (work queues), k_flush_rs chosen by plan_pass itself (208 x N = 190: its nontemporal instantiation), and two
           calls whose previous pass was a cadence's: a chained run's on the second stream (3 x N = 150) and a fused run's
           row-slab pass that formed W from V (208 x N = 190: w_from_v needs a panel launch outside the latency regime,
           B x ceil(n / 64) > 512 waves, AND the row-slab pass -- on the shipped defaults this bank is the smallest that has
           both).  Every case whose pass is k_flush_rs -- forced, chosen by the plan, behind the w_from_v pass -- is also held
           against a twin whose call runs k_flush (`pass_kernel` = 0), PATH_TOL = 1e-11 on every piece.
           Static shares (a few long trajectories, from N = 700 x 3 with forced workgroups) lie beyond this module's sizes.
  life     after the D = 33 direct and the D = 32 linear call: one step(), then 10 steps of the uploaded stream, against the
           oracle continued from the model.

Every case is the model (Joseph form) applied to state() taken just before the call -- from a twin driven identically where
ranks must be pending or the last pass must not be followed by a download -- under parity_blocks.assert_update_close at
TIGHT = 1e-9 on every piece.  Which instantiation ran is inferred from ekf_last_pass's k-tile count (kpad / 4) and the launch
from profile class 4 / 5; the closing test asserts that the kpad range of all four caps of both kernels and every pass form
were reached."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import parity_blocks as pb
from tests import update_cases as uc
from tests.gpu_support import same, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
PATH_TOL = 1e-11        # between two forms of the covariance pass, block-wise (the project states the same bits)
FORMS = ("k_flush", "k_flush streaming", "k_flush_rs forced B=3", "k_flush_rs forced B=8", "k_flush_rs auto",
         "behind a chained run", "behind a w_from_v pass")
REACHED = {"linear": set(), "direct": set(), "forms": set()}
RAN = set()
RESULTS = []


def make_bank(sd, base, steps=None):
    """The base's bank: every stream uploaded whole, its first `steps` steps (default: the base's) run, nothing downloaded."""
    B = uc.BASES[base][5]
    streams = [uc.stream(base, b) for b in range(B)]
    f = sd.EkfSlam(len(streams[0][0]), batch=B)
    for b, s in enumerate(streams):
        f.set_state_diag(s[0], s[1], b)
    f.stream_upload(*[np.stack([s[i] for s in streams], 1) for i in range(2, 7)])
    f.stream_run(0, uc.steps_of(base) if steps is None else steps)
    assert sd.load_library().ekf_debug_small_launches(f._h) == 0            # the general kernels
    return f


def profiled(f):
    f.set_option("profile_kernels", 1)
    f.profile_enable(True)


def last_pass(sd, f):
    """(kernel name, k-tiles) of the last covariance pass."""
    k, t, st = C.c_int(), C.c_int(), C.c_int()
    assert sd.load_library().ekf_last_pass(f._h, C.byref(k), C.byref(t), C.byref(st)) == 0
    return f.last_pass(), t.value


def call_linear(f, meas, modes, gate=None, b=None):
    """One update_linear: `meas` per trajectory (or trajectory b's alone), every entry in the same mode."""
    mode = modes if isinstance(modes, str) else modes[0]
    if b is not None or f.batch == 1:
        lms, H, R, r = meas if b is not None else meas[0]
        return f.update_linear(lms, H, R, gate=gate, b=0 if b is None else b, **{mode: r})
    return f.update_linear([m[0] for m in meas], [m[1] if len(m[3]) else None for m in meas],
                           [m[2] if len(m[3]) else None for m in meas], gate=gate, **{mode: [m[3] for m in meas]})


def call_direct(f, fixes, gate=None):
    if f.batch == 1:
        return f.update_direct(*fixes[0], gate=gate)
    return f.update_direct([x[0] for x in fixes], [x[1] for x in fixes], [x[2] for x in fixes], gate=gate)


def judge(sd, f, b, before, kind, payload, res, name, innovation=False, gate=np.inf):
    """Trajectory b after the call against the model applied to `before`; returns (state, the model's result)."""
    if kind == "linear":
        want = uc.linear_reference(before, payload, innovation, gate)
        touched, cross_tol = [int(l) for l in payload[0]], TIGHT
    else:
        want = uc.direct_reference(before, payload, gate)
        touched, cross_tol = [int(x) for x in payload[0] if x >= 0], None
    got = f.state(b)
    assert bool(res.applied[b]) == want[4] and res.dof[b] == want[3], (name, b, res.applied[b], res.dof[b], want[3:])
    if want[3]:
        assert res.nis[b] == pytest.approx(want[2], rel=1e-9), (name, b)
    if not want[4]:
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[1], before[1]), f"{name}: a rejected trajectory moved"
    err = pb.assert_update_close(got, want, before, touched, uc.INIT_VAR, TIGHT, what=f"{name} b={b}: ", first_cross_tol=cross_tol)
    worst = max((v, p) for p, v in err.items() if p in pb.PIECES)
    kernel, tiles = last_pass(sd, f)
    line = f"{name} b={b} D={want[3]}: worst {worst[1]}={worst[0]:.2e}  [{pb.fmt_update(err)}]  pass {kernel} k-tiles {tiles}"
    print("UPDATE_ROWS", line)
    RESULTS.append(line)
    return got, want


def instantiation(sd, f, kind, d_max):
    """The row cap the call's kernel must have been instantiated for, INFERRED from what the API exposes: the pass behind the
    call applied kpad / 4 k-tiles (ekf_last_pass), kpad the bank's largest D padded to 4, and profile class 4 / 5 counts one
    launch.  The cap itself is update_cases.rows_cap of that kpad -- this suite's copy of front_rows_cap
    (csrc/ekf_host_plan.h), the one argument ekf_api.hip hands the launcher; the template that ran is not observed, and a
    cap larger than kpad needs computes the same and would pass unseen."""
    _, tiles = last_pass(sd, f)
    assert tiles == (d_max + 3) // 4, (tiles, d_max)
    assert f.profile_read_class(4 if kind == "direct" else 5)[1] == 1
    cap = uc.rows_cap(4 * tiles, kind == "direct")
    REACHED[kind].add(cap)
    return cap


# ---- rows: one trajectory, every D ----
@pytest.mark.parametrize("D,k,mode", uc.LINEAR_ROWS)
def test_linear_rows(sd, D, k, mode):
    meas = uc.linear_case("n40", 0, D, k, mode)
    name = f"linear D={D} k={k} {mode}"
    with make_bank(sd, "n40") as f:
        before = f.state(0)
        profiled(f)
        res = call_linear(f, [meas], mode)
        cap = instantiation(sd, f, "linear", D)
        assert cap == uc.rows_cap(D, False) and res.applied[0] and res.dof[0] == D
        judge(sd, f, 0, before, "linear", meas, res, name, innovation=mode == "innovation")
        assert last_pass(sd, f)[0].startswith("ekf::k_flush<")
    RAN.add(name)


@pytest.mark.parametrize("D", sorted(uc.DIRECT_FIXES))
def test_direct_rows(sd, D):
    fix = uc.direct_case("n40", 0, D)
    name = f"direct D={D}"
    with make_bank(sd, "n40") as f:
        before = f.state(0)
        profiled(f)
        res = call_direct(f, [fix])
        cap = instantiation(sd, f, "direct", D)
        assert cap == uc.rows_cap(D, True) and res.applied[0] and res.dof[0] == D
        judge(sd, f, 0, before, "direct", fix, res, name)
        assert last_pass(sd, f)[0].startswith("ekf::k_flush<")
    RAN.add(name)


# ---- ragged banks ----
def ragged_payloads(kind, which):
    return uc.ragged_linear(which) if kind == "linear" else uc.ragged_direct(which)


def d_of(kind, payload):
    return len(payload[3]) if kind == "linear" else len(uc.dm.rows_of(payload[0]))


@pytest.mark.parametrize("kind", ["linear", "direct"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_ragged_bank(sd, kind, which):
    """(a) D = (1 | 2, 32 | 33, 0, 9): a small D inside the largest instantiation, dstride = 32 and lstride = 16 (stride 16 for
    the fixes) far above its own counts.  (b) D = (5, 8, 2, 7): cap 8, trajectory 2 ten sigma off under the 0.99 chi-square gate
    of its 2 rows -- rejected, bit for bit."""
    from scipy.stats import chi2
    payloads = ragged_payloads(kind, which)
    ds = [d_of(kind, p) for p in payloads]
    gate = [np.inf, np.inf, chi2.ppf(0.99, 2), np.inf] if which == "b" else None
    name = f"ragged {kind} ({which})"
    with make_bank(sd, "n40x4") as f:
        before = [f.state(b) for b in range(4)]
        profiled(f)
        res = call_linear(f, payloads, "innovation", gate) if kind == "linear" else call_direct(f, payloads, gate)
        cap = instantiation(sd, f, kind, max(ds))
        assert cap == ((36 if kind == "direct" else 32) if which == "a" else 8)
        assert list(res.dof) == ds
        assert list(res.applied) == [True, True, False, True]            # (trajectory 2: no rows in (a), rejected in (b))
        if which == "b":
            assert res.nis[2] > gate[2]
        for b in range(4):
            judge(sd, f, b, before[b], kind, payloads[b], res, name, innovation=True, gate=np.inf if gate is None else gate[b])
        assert same(f.state(2), before[2])
    RAN.add(name)


@pytest.mark.parametrize("kind", ["linear", "direct"])
def test_one_trajectory_alone_while_the_others_have_ranks_pending(sd, kind):
    """(c) a call that names trajectory 2 alone, 40 ranks pending in every trajectory of the bank: two passes (what was
    pending, then the call's), the others bit for bit a twin that was only flushed."""
    payload = uc.linear_case("n40x4", uc.LONE, *uc.PASS_LINEAR) if kind == "linear" else uc.direct_case("n40x4", uc.LONE, uc.PASS_DIRECT)
    name = f"lone {kind}"
    with make_bank(sd, "n40x4") as twin:
        twin.flush()
        before = [twin.state(b) for b in range(4)]
    with make_bank(sd, "n40x4") as f:
        profiled(f)
        assert f.profile_passes() == 0
        if kind == "linear":
            res = call_linear(f, payload, uc.PASS_LINEAR[2], b=uc.LONE)
        else:
            res = call_direct(f, [payload if b == uc.LONE else ([], [], []) for b in range(4)])
        assert f.profile_passes() == 2
        instantiation(sd, f, kind, d_of(kind, payload))
        assert list(res.applied) == [b == uc.LONE for b in range(4)]
        judge(sd, f, uc.LONE, before[uc.LONE], kind, payload, res, name)
        for b in range(4):
            if b != uc.LONE:
                assert same(f.state(b), before[b]), f"{name}: trajectory {b} differs from the flushed twin"
    RAN.add(name)


# ---- pass forms ----
def against_k_flush_twin(name, got, twin, bs):
    """The result behind a row-slab pass against that of a twin whose call ran the column-strip pass, per trajectory of `bs`:
    PATH_TOL on every piece, the never-observed landmarks bit for bit."""
    for b in bs:
        (mu, P), (tm, tP) = got[b], twin[b]
        err = pb.assert_filter_close(mu, P, tm, tP, pb.landmark_classes(tP, [], uc.INIT_VAR)[0], mean0=tm, diag0=np.diag(tP),
                                     tol=PATH_TOL, what=f"{name} b={b} against the k_flush twin: ")
        line = f"{name} b={b} against the k_flush twin: {pb.fmt(err)}"
        print("UPDATE_ROWS", line)
        RESULTS.append(line)


def pass_payloads(kind, base, bs):
    B = uc.BASES[base][5]
    if kind == "linear":
        empty = ([], np.zeros((0, 3)), np.zeros((0, 0)), np.zeros(0))
        return [uc.linear_case(base, b, *uc.PASS_LINEAR) if b in bs else empty for b in range(B)]
    return [uc.direct_case(base, b, uc.PASS_DIRECT) if b in bs else ([], [], []) for b in range(B)]


def pass_call(f, kind, payloads):
    return call_linear(f, payloads, uc.PASS_LINEAR[2]) if kind == "linear" else call_direct(f, payloads)


def bank_step(f, base, k):
    B = uc.BASES[base][5]
    s = [uc.stream(base, b) for b in range(B)]
    f.step(*[[x[i][k] for x in s] for i in range(2, 7)])


@pytest.mark.parametrize("kind", ["linear", "direct"])
@pytest.mark.parametrize("streaming", [0, 1])
def test_pass_form_column_strips(sd, kind, streaming):
    form = FORMS[streaming]
    payloads = pass_payloads(kind, "n40", [0])
    with make_bank(sd, "n40") as f:
        before = f.state(0)
        if streaming:
            f.set_option("pass_streaming", 1)
        res = pass_call(f, kind, payloads)
        kernel, _ = last_pass(sd, f)
        assert kernel.startswith("ekf::k_flush<") and kernel.endswith(", true>" if streaming else ", false>"), kernel
        judge(sd, f, 0, before, kind, payloads[0], res, f"{form} {kind}")
    REACHED["forms"].add(form)
    RAN.add(f"{form} {kind}")


@pytest.mark.parametrize("kind", ["linear", "direct"])
@pytest.mark.parametrize("base", ["n150x3", "n150x8"])
def test_pass_form_row_slabs_forced(sd, kind, base):
    """`pass_kernel` = 2 at N = 150 (active bound 243: two slabs): B = 3 has its slabs cut in chunks, B = 8 takes the work
    queues.  Against the model, and against a twin whose call runs the column-strip pass: PATH_TOL on every piece."""
    B = uc.BASES[base][5]
    form = FORMS[2] if B == 3 else FORMS[3]
    payloads = pass_payloads(kind, base, range(B))
    out = {}
    for pk in (2, 0):
        with make_bank(sd, base) as f:
            before = [f.state(b) for b in range(B)]
            f.set_option("pass_kernel", pk)
            res = pass_call(f, kind, payloads)
            kernel, _ = last_pass(sd, f)
            assert kernel.startswith("ekf::k_flush_rs<" if pk == 2 else "ekf::k_flush<"), kernel
            if pk == 2:
                for b in range(B):
                    judge(sd, f, b, before[b], kind, payloads[b], res, f"{form} {kind}")
            out[pk] = [f.state(b) for b in range(B)], before
    for b in range(B):
        assert same(out[2][1][b], out[0][1][b])                         # the twins entered the call with the same bits
    against_k_flush_twin(f"{form} {kind}", out[2][0], out[0][0], range(B))
    REACHED["forms"].add(form)
    RAN.add(f"{form} {kind}")


CHECKED, IDLE = range(4), range(4, 12)      # 208 x N = 190: trajectories that bring rows, and some of those that bring nothing


@pytest.mark.parametrize("kind", ["linear", "direct"])
def test_pass_form_row_slabs_chosen_by_the_plan(sd, kind):
    """208 x N = 190 on the shipped options: plan_pass sends the call's pass to k_flush_rs by itself -- the nontemporal
    instantiation, which no forced case launches.  24 steps of the stream and one step(): the download before the call applies
    what they left, so the call's predecessor is a plain pass.  Against the model, and against a twin of the same bank whose
    call runs the column-strip pass (`pass_kernel` = 0, set behind the download): PATH_TOL on every piece."""
    base, form = "n190x208", FORMS[4]
    payloads = pass_payloads(kind, base, CHECKED)
    out = {}
    for pk in (None, 0):
        with make_bank(sd, base, steps=24) as f:
            bank_step(f, base, 24)
            before = {b: f.state(b) for b in list(CHECKED) + list(IDLE)}
            if pk is not None:
                f.set_option("pass_kernel", pk)
            res = pass_call(f, kind, payloads)
            kernel, _ = last_pass(sd, f)
            assert list(np.flatnonzero(res.applied)) == list(CHECKED)
            if pk is None:
                assert kernel.startswith("ekf::k_flush_rs<") and kernel.endswith("false>"), kernel
                for b in CHECKED:
                    judge(sd, f, b, before[b], kind, payloads[b], res, f"{form} {kind}")
            else:
                assert kernel.startswith("ekf::k_flush<"), kernel
            out[pk] = {b: f.state(b) for b in before}, before
    for b in list(CHECKED) + list(IDLE):
        assert same(out[None][1][b], out[0][1][b])                      # the twins entered the call with the same bits
    for b in IDLE:
        assert same(out[None][0][b], out[None][1][b]), f"{form} {kind}: trajectory {b} brought nothing and moved"
        assert same(out[0][0][b], out[0][1][b]), f"{form} {kind}: trajectory {b} of the k_flush twin moved"
    against_k_flush_twin(f"{form} {kind}", out[None][0], out[0][0], CHECKED)
    REACHED["forms"].add(form)
    RAN.add(f"{form} {kind}")


@pytest.mark.parametrize("kind", ["linear", "direct"])
def test_call_behind_a_chained_run(sd, kind):
    """3 x N = 150, 30 steps = 3 whole cadences as a chained run: the last pass ran on the handle's second stream and nothing
    is pending; the call follows with no download in between (the state before it: a twin's).

    What is stale here, exactly: the predecessor is a plain k_flush that the chained run launched on the handle's SECOND
    stream, and no download has joined it, so the call's kernel and pass (on the first stream) are the first work ordered
    behind it; the active bounds and the pending pose noise on the device are what the last cadence's launches left, not what
    a flush or a download would have refreshed.  NOT stale: last_wv, shares and queue heads -- a k_flush has none of them
    (ekf_last_pass names k_flush before and behind the call).  Of those three the w_from_v case below has the first and the
    last; static shares lie beyond this module's sizes.  The shape is the forced B = 3 bank reused; any bank whose run
    ekf_debug_chained counts gets here, and this one is not claimed to be the smallest such."""
    base, form = "n150x3", FORMS[5]
    lib = sd.load_library()
    payloads = pass_payloads(kind, base, range(3))
    with make_bank(sd, base) as twin:
        assert lib.ekf_debug_chained(twin._h) > 0
        before = [twin.state(b) for b in range(3)]
    with make_bank(sd, base) as f:
        assert lib.ekf_debug_chained(f._h) > 0
        profiled(f)
        res = pass_call(f, kind, payloads)
        assert f.profile_passes() == 1                                       # nothing was pending: the call's own pass alone
        kernel, _ = last_pass(sd, f)
        assert kernel.startswith("ekf::k_flush<"), kernel
        for b in range(3):
            judge(sd, f, b, before[b], kind, payloads[b], res, f"{form} {kind}")
    REACHED["forms"].add(form)
    RAN.add(f"{form} {kind}")


@pytest.mark.parametrize("kind", ["linear", "direct"])
def test_call_behind_a_w_from_v_pass(sd, kind):
    """208 x N = 190, 25 steps of m = 8 = 5 whole cadences of a fused run: the last cadence's pass is the row-slab form that
    built its W fragments from V (ekf_debug_last_pass_wv), on the work queues; the call's pass finds the W the call wrote, a
    cleared w_from_v and fresh queue heads -- or it does not, and the pieces show it."""
    base, form = "n190x208", FORMS[6]
    lib = sd.load_library()
    payloads = pass_payloads(kind, base, CHECKED)
    with make_bank(sd, base) as twin:
        before = {b: twin.state(b) for b in list(CHECKED) + list(IDLE)}
    out = {}
    for pk in (None, 0):
        with make_bank(sd, base) as f:
            kernel, _ = last_pass(sd, f)
            assert kernel.startswith("ekf::k_flush_rs<") and lib.ekf_debug_last_pass_wv(f._h) == 1, kernel
            if pk is not None:
                f.set_option("pass_kernel", pk)                              # behind the run: the fused run itself is the same
            profiled(f)
            res = pass_call(f, kind, payloads)
            assert f.profile_passes() == 1                                   # nothing was pending: the call's own pass alone
            kernel, _ = last_pass(sd, f)
            assert lib.ekf_debug_last_pass_wv(f._h) == 0
            if pk is None:
                assert kernel.startswith("ekf::k_flush_rs<"), kernel
                for b in CHECKED:
                    judge(sd, f, b, before[b], kind, payloads[b], res, f"{form} {kind}")
            else:
                assert kernel.startswith("ekf::k_flush<"), kernel
            out[pk] = {b: f.state(b) for b in before}
            for b in IDLE:
                assert same(out[pk][b], before[b]), f"{form} {kind}: trajectory {b} brought nothing and moved (pass_kernel {pk})"
    against_k_flush_twin(f"{form} {kind}", out[None], out[0], CHECKED)
    REACHED["forms"].add(form)
    RAN.add(f"{form} {kind}")


# ---- life goes on ----
@pytest.mark.parametrize("kind", ["linear", "direct"])
def test_life_goes_on_behind_the_largest_call(sd, kind):
    """After the D = 32 linear / D = 33 direct call: one step(), then 10 steps of the uploaded stream, against the oracle
    continued from the model's result -- a stale active bound, pose noise or queue head would show here and not in the call."""
    base = "n40"
    if kind == "linear":
        D, k, mode = next(c for c in uc.LINEAR_ROWS if c[0] == 32)
        payload = uc.linear_case(base, 0, D, k, mode)
    else:
        payload, mode = uc.direct_case(base, 0, 33), "z"
    s = uc.stream(base, 0)
    first = uc.steps_of(base)
    name = f"life {kind}"
    with make_bank(sd, base) as f:
        before = f.state(0)
        res = call_linear(f, [payload], mode) if kind == "linear" else call_direct(f, [payload])
        _, want = judge(sd, f, 0, before, kind, payload, res, name, innovation=mode == "innovation")
        om, oP = want[0], want[1]
        f.step(*[s[i][first] for i in range(2, 7)])
        f.stream_run(first + 1, 10)
        cfg = orc.EkfConfig()
        for j in range(first, first + 11):
            om, oP = orc.ekf_step_dense(om, oP, s[2][j], s[3][j], s[4][j], s[5][j], s[6][j], cfg)
        mu, P = f.state(0)
        assert f.flags(0) == 0
        err = pb.assert_filter_close(mu, P, om, oP, pb.landmark_classes(oP, [], uc.INIT_VAR)[0], mean0=before[0],
                                     diag0=np.diag(before[1]), tol=TIGHT, what=f"{name}, 11 steps on: ")
        print(f"UPDATE_ROWS {name}, 11 steps on: {pb.fmt(err)}  pass {f.last_pass()}")
        RESULTS.append(f"{name}, 11 steps on: {pb.fmt(err)}")
    RAN.add(name)


def expected():
    names = {f"linear D={D} k={k} {mode}" for D, k, mode in uc.LINEAR_ROWS} | {f"direct D={D}" for D in uc.DIRECT_FIXES}
    for kind in ("linear", "direct"):
        names |= {f"ragged {kind} (a)", f"ragged {kind} (b)", f"lone {kind}", f"life {kind}"} | {f"{form} {kind}" for form in FORMS}
    return names


def test_module_reached_every_instantiation_and_pass_form():
    """Not vacuous: the calls of this module had kpad in the range of each of the four row caps of k_linear and of k_direct
    (inferred from the pass's k-tile count, `instantiation`; the template itself is not observed), and every named form of the
    pass ran behind both kernels (the kernel's name from ekf_last_pass).  Like test_module_reached_every_promise this needs the
    whole module in one process: under -k or a split over workers it skips and the coverage claim is not made."""
    if RAN != expected():
        pytest.skip("needs every case of the module in the same run")
    print("\n".join("UPDATE_ROWS_SUMMARY " + r for r in RESULTS))
    assert REACHED["linear"] == {4, 8, 16, 32} and REACHED["direct"] == {4, 8, 16, 36}, REACHED
    assert REACHED["forms"] == set(FORMS), set(FORMS) - REACHED["forms"]
