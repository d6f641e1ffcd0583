"""The unit hand-over of the row-slab covariance pass (k_flush_rs, slam-duckietown_amd/csrc/ekf_kernels.hip): a workgroup
takes its next unit while the one in hand still runs -- the queue pop is issued one or two tiles before the unit's end (in
front of the prologue for a unit of one strip), its answer is read just before the drain, and the next piece of a static
share is read a unit ahead.

Every case compares the row-slab pass with the column-strip pass (k_flush, untouched, the reference) BIT FOR BIT on
`state()`, both forced through `pass_kernel`, the row-slab pass with `w_from_v` off and on; every trajectory flag must be
0.  Every case runs at least 3 passes (the panelled single trajectory: 2), so that what one pass wrote is what the next
reads.  The shapes are the smallest at which the hand-over can go wrong: many units of 1-2 strips per workgroup, units
stolen from other queues, slabs cut in chunks, ragged banks (units without work, waves without tiles), the active bound
growing between passes, static shares, the column-panel layout, every rank count of one instantiation.
"""
import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.gpu_support import sd  # noqa: F401
from tests.streams import dense_start

pytestmark = pytest.mark.gpu


def bank_stream(Ns, steps, m, seed, visible=None):
    """One stream per trajectory (trajectory b has Ns[b] landmarks), `m` observations per step; `visible(k, N)`: the
    observations of step k come from the landmarks [0, visible(k, N)) (default: all of them)."""
    B = len(Ns)
    rng = np.random.default_rng(seed)
    cfg = orc.EkfConfig()
    world = [orc.synthetic_world(N, seed + 1 + t) for t, N in enumerate(Ns)]
    lin = np.full((steps, B), 0.004)
    ang = np.where(np.arange(steps)[:, None] % 7 == 6, 0.005, 0.02) * np.ones((1, B))
    idx = np.zeros((steps, B, m), dtype=np.int32)
    zr, zb = np.zeros((steps, B, m)), np.zeros((steps, B, m))
    pose = [np.zeros(3) for _ in range(B)]
    for k in range(steps):
        for b, N in enumerate(Ns):
            pose[b], _ = orc.motion_model(pose[b], lin[k, b], ang[k, b], cfg)
            hi = N if visible is None else max(m, min(N, int(visible(k, N))))
            vis = rng.choice(hi, size=m, replace=False)
            d = world[b][1][vis] - pose[b][0:2]
            cth, sth = np.cos(pose[b][2]), np.sin(pose[b][2])
            xr = cth * d[:, 0] + sth * d[:, 1] + rng.normal(0, 0.01, m)
            yr = -sth * d[:, 0] + cth * d[:, 1] + rng.normal(0, 0.01, m)
            idx[k, b], zr[k, b], zb[k, b] = vis, np.sqrt(xr ** 2 + yr ** 2), np.arctan2(yr, xr)
    return [w[2] for w in world], [w[3] for w in world], lin, ang, idx, zr, zb


def run_bank(sd, Ns, stream, options, kernel, wv, diag=False, seed=0, passes=3):
    """The whole stream as fused cadences on one handle with the pass forced to `kernel`; [(mean, cov)] per trajectory."""
    means, diags, lin, ang, idx, zr, zb = stream
    B = len(Ns)
    n_max = 3 + 2 * max(Ns)
    with sd.EkfSlam(n_max, batch=B) as f:
        for name, value in (("pass_kernel", kernel), ("w_from_v", wv)) + tuple(options):
            f.set_option(name, value)
        for b, N in enumerate(Ns):
            if diag:
                f.set_state_diag(means[b], diags[b], b)
            else:
                f.set_state(means[b], dense_start(3 + 2 * N, seed + b), b)
        f.run_stream(lin, ang, idx, zr, zb)
        out = [f.state(b) for b in range(B)]
        assert [f.flags(b) for b in range(B)] == [0] * B
        assert f.cadence_counters()[0] >= passes
        assert ("k_flush_rs<" if kernel == 2 else "k_flush<") in f.last_pass()
        if kernel == 2:
            assert f.last_pass().endswith("true>" if wv else "false>"), f.last_pass()
        shares = sd.load_library().ekf_debug_last_pass_shares(f._h)
        print(f"B={B} n_max={n_max} {f.last_pass()} passes={f.cadence_counters()[0]} share pieces={shares}")
    return out, shares


def check_bank(sd, Ns, steps, m, seed, options=(), diag=False, visible=None, passes=3, shares=False):
    stream = bank_stream(Ns, steps, m, seed, visible)
    if "active_bound" not in dict(options):
        options = (("active_bound", 0),) + tuple(options)
    # every solve behind its pass: beside a column-strip pass the solves of a small bank are chained (other operations,
    # equal to rounding only), and only a pass that follows its panel launch at once forms W from V
    # (... and only behind the panel launch's independent-wave shapes: forced, so that `w_from_v` is taken at every size)
    options = (("lookahead", 0), ("panel_shape", 3)) + tuple(options)
    ref, _ = run_bank(sd, Ns, stream, options, 0, 0, diag, seed, passes)
    for wv in (0, 1):
        got, pieces = run_bank(sd, Ns, stream, options, 2, wv, diag, seed, passes)
        assert (pieces >= 1) == shares, (wv, pieces)
        for b in range(len(Ns)):
            assert np.array_equal(ref[b][0], got[b][0]), (wv, b)
            assert np.array_equal(ref[b][1], got[b][1]), (wv, b)


@pytest.mark.parametrize("N,B", [(265, 40), (130, 64)])
def test_many_short_units_per_workgroup(sd, N, B):
    """n = 533 (5 slabs of 9, 7, 5, 3, 1 strips, the last with 21 rows) x 40 and n = 263 x 64: a workgroup walks several
    units of 1-2 strips, so the pop goes out in front of the prologue and is read one tile later."""
    check_bank(sd, [N] * B, 15, 8, 7000 + N)


@pytest.mark.parametrize("B", [9, 13, 30])
def test_units_taken_from_other_queues(sd, B):
    """A batch that is no multiple of 8 at N = 700: the last trajectories are dealt over all queues (9: half slabs, 13 and
    30: whole slabs) and the workgroups of a queue that has run dry take units from the other XCDs' queues."""
    check_bank(sd, [700] * B, 15, 8, 7100 + B)


@pytest.mark.parametrize("chunk", [3, 7])
def test_slabs_cut_in_chunks(sd, chunk):
    """`pass_chunk` 3 and 7 at N = 1300 x 5 (41 strips in the longest slab): nch > 1, chunks that start beyond the end of
    a short slab (units without work pop their successor at once)."""
    check_bank(sd, [1300] * 5, 15, 8, 7200 + chunk, options=(("pass_chunk", chunk),))


@pytest.mark.parametrize("B", [6, 11])
def test_ragged_banks(sd, B):
    """Trajectories of n = 67 (smaller than a slab) to 1499 in one bank: units whose slab lies beyond the trajectory's
    rows, waves without tiles, last slabs of a few rows -- as the queues' uniform chunks (6) and as dealt half slabs (11)."""
    sizes = [32, 748, 100, 531, 265, 400, 64, 700, 33, 300, 200]
    check_bank(sd, sizes[:B], 15, 8, 7300 + B)


def test_active_bound_growing_between_passes(sd):
    """The active bound on, block-diagonal start, the observed landmarks reaching further with every step: the rows the
    pass covers (neff < nact) grow from pass to pass."""
    steps = 20
    check_bank(sd, [700] * 16, steps, 8, 7400, options=(("active_bound", 1),), diag=True,
               visible=lambda k, N: N * (k + 2) // (steps + 1), passes=4)


def test_static_shares(sd):
    """N = 2100 x 3 on 64 workgroups: equal static shares (mode 4: no queue; the next piece is read a unit ahead), on the
    column-panel layout."""
    check_bank(sd, [2100] * 3, 15, 8, 7500, options=(("pass_workgroups", 64),), shares=True)


def test_column_panel_layout(sd):
    """n = 4203 > 4096 (the size tests/test_gpu_layout.py crosses the panel boundary with), one trajectory, 2 passes."""
    check_bank(sd, [2100], 10, 8, 7600, passes=2)


@pytest.mark.parametrize("streaming", [0, 1])
def test_all_rank_counts_of_one_instantiation(sd, streaming):
    """`rank_limit` 16, 48, 80 at N = 531 x 3 on the per-step path (a pass per 1, 3, 5 steps: 15, 5, 3 passes), both
    cache policies -- the shape that exposed the store hazard (stb16)."""
    N, B, m, steps = 531, 3, 8, 15
    n = 3 + 2 * N
    means, _, lin, ang, idx, zr, zb = bank_stream([N] * B, steps, m, 7700)
    starts = [dense_start(n, 7710 + b) for b in range(B)]
    for limit in (16, 48, 80):
        out = {}
        for kernel in (0, 2):
            with sd.EkfSlam(n, batch=B) as f:
                for name, value in (("pass_kernel", kernel), ("rank_limit", limit), ("pass_streaming", streaming),
                                    ("active_bound", 0)):
                    f.set_option(name, value)
                for b in range(B):
                    f.set_state(means[b], starts[b], b)
                for k in range(steps):
                    f.step(lin[k], ang[k], list(idx[k]), list(zr[k]), list(zb[k]))
                out[kernel] = [f.state(b) for b in range(B)]
                assert [f.flags(b) for b in range(B)] == [0] * B
                assert ("k_flush_rs<" if kernel == 2 else "k_flush<") in f.last_pass()
        for b in range(B):
            assert np.array_equal(out[0][b][0], out[2][b][0]), (limit, b)
            assert np.array_equal(out[0][b][1], out[2][b][1]), (limit, b)
