"""GPU: the three orders a run's cadences are enqueued in (csrc/ekf_host_plan.h: plan_cadence_launches -- chained solves, the
look-ahead, everything one behind the other), taken one after the other on ONE handle: a stream run in pieces, the order
switched by options between the pieces, nothing flushed in between beyond what ekf_stream_run does itself.  The counters,
parities and serials the orders share (CadRun) are carried from piece to piece, both logs are on and their rings wrap.

The references are the per-step kernels (`fused_cadence` = 0) and the oracle, never the cadence path itself.  Tolerances are
the constants of test_gpu_cadence.py: PATH_TOL, relative Frobenius, between the two paths -- the final states, and every logged
step's rows of each trajectory (y, S and NIS of its landmark updates; its pose mean and pose block), each array by itself --
and TIGHT against the oracle."""
import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.gpu_support import counters, sd  # noqa: F401
from tests.streams import dense_start

pytestmark = pytest.mark.gpu

PATH_TOL = 1e-11        # tests/test_gpu_cadence.py's two constants, restated: no file imports from a test module
TIGHT = 1e-9            # (tests/test_imports_cpu.py)

DEFAULTS = (("lookahead", 1), ("chain", 1))
LOOKAHEAD = (("lookahead", 1), ("chain", 0))
SERIAL = (("lookahead", 0), ("chain", 1))
STEPS, PIECE, M, LOG_CAP = 60, 15, 8, 40              # 15 steps x 8 landmarks = three full cadences per piece; the rings hold 40 of 60 steps


def run(sd, n, streams, starts, args, pieces):
    """The stream on one handle: in pieces with the given options (and the counters' moves asserted) or, `pieces` None, whole
    on the per-step kernels.  Returns the states, the innovation log and the pose log."""
    B = len(streams)
    with sd.EkfSlam(n, batch=B) as f:
        f.set_option("active_bound", 0)
        if pieces is None:
            f.set_option("fused_cadence", 0)
        f.log_innovations(LOG_CAP)
        f.log_poses(LOG_CAP)
        for b in range(B):
            f.set_state(streams[b][0], starts[b], b)
        f.stream_upload(*args)
        if pieces is None:
            f.stream_run(0, STEPS)
            assert counters(sd, f).cadences == 0
        else:
            for i, (opts, moved) in enumerate(pieces):
                for name, value in opts:
                    f.set_option(name, value)
                c0 = counters(sd, f)
                f.stream_run(i * PIECE, PIECE)
                c1 = counters(sd, f)
                got = (c1.cadences - c0.cadences, c1.lookaheads - c0.lookaheads, c1.chained - c0.chained)
                assert got == moved, (i, got, moved)
        out = [f.state(b) for b in range(B)]
        assert [f.flags(b) for b in range(B)] == [0] * B
        return out, f.innovations(), f.poses()


def rows_err(a, b, axes):
    """Relative Frobenius error of every logged step's rows of every trajectory: a, b (K, B, ...), `axes` the rows' own."""
    return np.sqrt(np.sum((a - b) ** 2, axis=axes) / np.sum(b ** 2, axis=axes))


def check_logs(got, ref):
    (_, gi, gp), (_, ri, rp) = got, ref
    assert gi.steps.tolist() == ri.steps.tolist() == list(range(STEPS - LOG_CAP, STEPS))
    assert (gi.m == ri.m).all() and (gi.idx == ri.idx).all() and (gi.m == M).all()            # (every entry of a row is in use)
    assert gp.first == rp.first == STEPS - LOG_CAP and gp.mean.shape == rp.mean.shape == (LOG_CAP, gi.m.shape[1], 3)
    worst = {"y": rows_err(gi.y, ri.y, (-2, -1)).max(), "S": rows_err(gi.S, ri.S, (-3, -2, -1)).max(),
             "NIS": rows_err(gi.nis, ri.nis, -1).max(), "pose mean": rows_err(gp.mean, rp.mean, -1).max(),
             "pose block": rows_err(gp.cov, rp.cov, (-2, -1)).max()}
    print("log rows against the per-step path, worst step: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v < PATH_TOL for v in worst.values()), worst


@pytest.mark.parametrize("N,B,pieces", [
    # the smallest state at which options alone select all three orders (8 n^2 >= 48 MB): chained, look-ahead, serial, chained
    (1250, 1, ((DEFAULTS, (3, 2, 2)), (LOOKAHEAD, (3, 2, 0)), (SERIAL, (3, 0, 0)), (DEFAULTS, (3, 2, 2)))),
    # the smallest state with more than one trajectory: chained and serial in turn
    (100, 2, ((DEFAULTS, (3, 2, 2)), (SERIAL, (3, 0, 0)), (DEFAULTS, (3, 2, 2)), (SERIAL, (3, 0, 0)))),
])
def test_orders_in_turn_on_one_handle(sd, N, B, pieces):
    n = 3 + 2 * N
    streams = [orc.synthetic_stream(N, STEPS, M, 4300 + t) for t in range(B)]
    starts = [dense_start(n, 4400 + t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    got = run(sd, n, streams, starts, args, pieces)
    ref = run(sd, n, streams, starts, args, None)
    for b in range(B):
        e_mu, e_P = orc.rel_fro(got[0][b][0], ref[0][b][0]), orc.rel_fro(got[0][b][1], ref[0][b][1])
        print(f"trajectory {b}: against the per-step path mean {e_mu:.3g} covariance {e_P:.3g}")
        assert e_mu < PATH_TOL and e_P < PATH_TOL
    check_logs(got, ref)
    cfg = orc.EkfConfig()
    for b in range(B):
        s = streams[b]
        om, oP = s[0].copy(), starts[b].copy()
        for k in range(STEPS):                             # (the O(n^2) form of the oracle)
            om, oP = orc.ekf_step_structured(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
        e_mu, e_P = orc.rel_fro(got[0][b][0], om), orc.rel_fro(got[0][b][1], oP)
        print(f"trajectory {b}: against the oracle mean {e_mu:.3g} covariance {e_P:.3g}")
        assert e_mu < TIGHT and e_P < TIGHT
