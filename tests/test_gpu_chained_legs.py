"""The chained benchmark legs as bench.py times them, checked against the oracle block by block (tests/parity_blocks.py).

Round 6 chains the cadence solves: each cadence's solve starts from a block `k_chain_cad` forms from the previous cadence's
records instead of gathering it again.  bench.py times that path for hundreds of steps at N = 500, 2000 and 8000; these
tests run the same streams the same way (`time_filter`: set_state_diag, stream_upload, the warm-up piece, flush, the
profiling event pairs between the chained launches, the timed piece, flush) and assert, per leg: the chained solves
counted, no flags, the pass kernel the leg reports, the marginals after the warm-up piece and the whole state at the end
against `oracle.ekf_step_structured`, piece by piece.  Then what the benchmark streams never do -- revisit a landmark of
the previous cadence, of the same cadence and of 200 steps ago at N = 2000, updates scattered over both column panels of
the row-slab pass at N = 8000 -- and chained handles side by side on two host threads.

The oracle runs in worker processes (started fresh, never touching the GPU), submitted when the module's first test starts.
"""
import concurrent.futures as cf
import multiprocessing as mp
import threading

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import parity_blocks as pb
from tests.gpu_support import counters, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
PATH_TOL = 1e-11
M = 8


# ----------------------------------------------------------------------------------------------------------------------
# streams (host only: also imported by the oracle workers)
# ----------------------------------------------------------------------------------------------------------------------
# leg -> (N, warm-up steps, timed steps, (m_lo, m_hi) or None, active_bound), as bench.py's secondary legs run them
LEGS = {
    "single_trajectory": (2000, 20, 200, None, 0),
    "config2": (500, 20, 500, None, 0),
    "x1_m0to3": (2000, 60, 600, (0, 3), 0),
    "config5_skip_unobserved": (8000, 20, 100, None, 1),
    "config5_dense": (8000, 20, 100, None, 0),
}


def leg_stream(name):
    """bench.py's make_streams for trajectory 0: mean0, diag0, lin, ang, idx, zr, zb, m (None for a constant m)."""
    import slam_duckietown_amd.synthetic as syn
    N, warm, steps, variable, _ = LEGS[name]
    if variable:
        return syn.variable_stream(N, warm + steps, variable[0], variable[1], 0)
    return syn.synthetic_stream(N, warm + steps, M, 0) + (None,)


def profile_stride(name):
    """The stride time_filter sets for the timed piece."""
    _, _, steps, variable, _ = LEGS[name]
    expect = steps * (M if variable is None else (variable[0] + variable[1]) / 2.0) / 40.0
    return 4 if expect >= 16 else (2 if expect >= 4 else 1)


def scheduled_stream(N, schedule, trajectory_id=0):
    """The world, kinematics and noise of synthetic.variable_stream, measuring the landmarks `schedule[k]` (distinct
    within a step) at step k.  -> mean0, diag0, lin, ang, idx, zr, zb."""
    import slam_duckietown_amd.synthetic as syn
    rng, lm, mean0, diag0 = syn._world(N, trajectory_id)
    steps, m = len(schedule), len(schedule[0])
    lin = np.full(steps, 0.004)
    ang = np.full(steps, 0.02)
    ang[9::10] = 0.005
    idx = np.asarray(schedule, dtype=np.int32)
    zr, zb = np.zeros((steps, m)), np.zeros((steps, m))
    pose = np.zeros(3)
    for k in range(steps):
        pose = syn._advance(pose, lin[k], ang[k])
        assert len(set(idx[k].tolist())) == m
        d = lm[idx[k]] - pose[0:2]
        c, s = np.cos(pose[2]), np.sin(pose[2])
        xr = c * d[:, 0] + s * d[:, 1] + rng.normal(0.0, 0.01, m)
        yr = -s * d[:, 0] + c * d[:, 1] + rng.normal(0.0, 0.01, m)
        zr[k] = np.sqrt(xr ** 2 + yr ** 2)
        zb[k] = np.arctan2(yr, xr)
    return mean0, diag0, lin, ang, idx, zr, zb


def revisit_schedule(steps=300, N=2000):
    """m = 8 per step at N = 2000, cadences of 5 steps (40 updates): 4 new landmarks in sweep order; 2 observed in the
    previous cadence; 1 from about 200 steps earlier (loop closure: from step k // 2 before step 200); 1 observed earlier
    in the same cadence (in the previous step when the step opens a cadence).  The first cadence observes 8 new ones."""
    new = lambda k: [4 * k + j for j in range(4)]                         # noqa: E731
    out = []
    for k in range(steps):
        c = k // 5
        if c == 0:
            out.append(new(k) + [4 * steps + 4 * k + j for j in range(4)])
            continue
        prev = [new(k - 5)[0], new(5 * (c - 1) + (k + 2) % 5)[1]]
        loop = new(k - 200 if k >= 200 else k // 2)[2]
        same = new(5 * c)[3] if k > 5 * c else new(k - 1)[3]
        out.append(new(k) + prev + [loop, same])
    assert max(max(r) for r in out) < N
    return out


def scattered_schedule(steps=40, N=8000):
    """synthetic_stream's sweep scattered over the whole state, as test_max_size_n8000_three_steps does."""
    return [[(int(M * k + j) * 997 + 13) % N for j in range(M)] for k in range(steps)]


# ----------------------------------------------------------------------------------------------------------------------
# oracle workers
# ----------------------------------------------------------------------------------------------------------------------
def _run_oracle(om, oP, s, first, count, m=None):
    cfg = orc.EkfConfig()
    for k in range(first, first + count):
        mk = s[4].shape[1] if m is None else int(m[k])
        om, oP = orc.ekf_step_structured(om, oP, s[2][k], s[3][k], s[4][k][:mk], s[5][k][:mk], s[6][k][:mk], cfg)
    return om, oP


def _marg(oP, N):
    r = 3 + 2 * np.arange(N)
    return oP[:3, :3].copy(), np.stack([np.stack([oP[r, r], oP[r, r + 1]], -1), np.stack([oP[r + 1, r], oP[r + 1, r + 1]], -1)], -2)


def oracle_job(job):
    """(worker process) -> the pieces a test compares.  Legs: the pose block and landmark blocks after the warm-up piece,
    the state at the end (on the active part -- a closed system -- at N = 8000)."""
    if job in ("single_trajectory", "config2", "x1_m0to3", "config5"):
        name = "config5_dense" if job == "config5" else job
        N, warm, steps, _, _ = LEGS[name]
        s = leg_stream(name)
        top = 3 + 2 * (int(pb.observed_landmarks(s[4], s[7]).max()) + 1) if N == 8000 else len(s[0])
        om, oP = s[0][:top].copy(), np.diag(s[1][:top])
        om, oP = _run_oracle(om, oP, s, 0, warm, s[7])
        warm_blocks = _marg(oP, (top - 3) // 2)
        om, oP = _run_oracle(om, oP, s, warm, steps, s[7])
        return {"warm": warm_blocks, "final": (om, oP)}
    if job == "revisits_n2000":
        s = scheduled_stream(2000, revisit_schedule())
        return _run_oracle(s[0].copy(), np.diag(s[1]), s, 0, len(s[2]))
    if job == "scattered_n8000":
        s = scheduled_stream(8000, scattered_schedule())
        om, oP = _run_oracle(s[0].copy(), np.diag(s[1]), s, 0, len(s[2]))
        act = np.concatenate([np.arange(3), pb.landmark_rows(pb.observed_landmarks(s[4]))])
        return {"mean": om, "rows": oP[act].copy(), "diag": np.diag(oP).copy(), "rowsum": oP.sum(axis=1)}
    raise ValueError(job)


JOBS = ("x1_m0to3", "scattered_n8000", "revisits_n2000", "single_trajectory", "config5", "config2")


@pytest.fixture(scope="module")
def oracle():
    """Every oracle run of the module, submitted at once (longest first) to at most 4 fresh worker processes."""
    pool = cf.ProcessPoolExecutor(max_workers=4, mp_context=mp.get_context("spawn"))
    futures = {job: pool.submit(oracle_job, job) for job in JOBS}
    yield futures
    pool.shutdown(wait=True, cancel_futures=True)


# ----------------------------------------------------------------------------------------------------------------------
# C. the chained legs as benchmarked
# ----------------------------------------------------------------------------------------------------------------------
# leg -> (expected ekf_debug_chained: cadences - 1 per piece, the pass kernel the leg reports).  The kernels, from
# ekf_host_plan.h::plan_pass: one trajectory at N = 500 or 2000 moves 8 MB / 128 MB per pass, below the 192 MB from which the
# pass streams (nontemporal), and the row-slab form needs a streaming pass -> the column-strip k_flush; 80 pending ranks are
# 20 k-tiles, 15 in registers + 5 in LDS.  x1_m0to3: the last pass is the tail cadence's, at most 64 ranks (16 k-tiles).
# N = 8000, active bound on: 2 GB streams, but the 1923 active rows are 16 slabs, too few for the row-slab form ->
# k_flush<15, 5, true>; off: a few long trajectories on static shares, one CU left to the chained solve beside the pass
# (`beside`), column-panel layout beyond n = 4096, W not formed from V where a solve runs beside it.
EXPECT = {
    "single_trajectory": (3 + 39, "ekf::k_flush<15, 5, false>"),
    "config2": (3 + 99, "ekf::k_flush<15, 5, false>"),
    "x1_m0to3": (None, "ekf::k_flush<16, 0, false>"),
    "config5_skip_unobserved": (3 + 19, "ekf::k_flush<15, 5, true>"),
    "config5_dense": (3 + 19, "ekf::k_flush_rs<20, true, true, false>"),
}


@pytest.mark.parametrize("name", list(LEGS))
def test_chained_leg_as_benchmarked(sd, oracle, name):
    N, warm, steps, _, bound = LEGS[name]
    s = leg_stream(name)
    n = 3 + 2 * N
    mean0, diag0 = s[0], s[1]
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("active_bound", bound)
        f.set_state_diag(mean0, diag0)
        f.stream_upload(s[2], s[3], s[4], s[5], s[6], s[7])
        f.stream_run(0, warm)
        f.flush()
        pose_w, lms_w = (np.array(a) for a in f.marginals(0))             # read-only: the schedule stays as benchmarked
        cad_w = f.cadence_counters()
        chained_w = counters(sd, f).chained
        f.set_option("profile_stride", profile_stride(name))
        f.profile_enable(True)
        f.stream_run(warm, steps)
        f.flush()
        ms, timed = f.profile_read()
        passes = f.profile_passes()
        f.profile_enable(False)
        cad = f.cadence_counters()
        n_chained = counters(sd, f).chained
        kernel = f.last_pass()
        flags = f.flags()
        mu, P = f.state()
    print(f"\n{name}: cadences {cad_w} -> {cad}, chained {chained_w} -> {n_chained}, pass {kernel}, "
          f"{timed} of {passes} passes timed ({ms:.3f} ms)")
    assert flags == 0
    assert cad[1] == warm + steps                                         # every step ran in a fused cadence
    want, want_kernel = EXPECT[name]
    if want is None:                                                      # cadences - 1 per piece, two pieces
        want = cad[0] - 2
    assert (chained_w, n_chained) == (cad_w[0] - 1, want), (chained_w, n_chained, cad_w, cad)
    assert timed >= 1 and passes >= timed and ms > 0.0
    assert kernel == want_kernel

    res = oracle["config5" if N == 8000 else name].result()
    obs_w = pb.observed_landmarks(s[4][:warm], None if s[7] is None else s[7][:warm])
    ref_pose, ref_lms = res["warm"]
    r = 3 + 2 * obs_w
    ref_oP = np.zeros((len(ref_lms) * 2 + 3,) * 2)                       # the oracle's blocks, in a covariance's places
    ref_oP[:3, :3] = ref_pose
    ref_oP[r, r], ref_oP[r, r + 1] = ref_lms[obs_w, 0, 0], ref_lms[obs_w, 0, 1]
    ref_oP[r + 1, r], ref_oP[r + 1, r + 1] = ref_lms[obs_w, 1, 0], ref_lms[obs_w, 1, 1]
    e_w = pb.assert_marginals_close(pose_w, lms_w, ref_oP, obs_w, diag0=diag0, what=f"{name} after the warm-up: ")
    om, oP = res["final"]
    obs = pb.observed_landmarks(s[4], s[7])
    err = pb.assert_filter_close(mu, P, om, oP, obs, mean0=mean0, diag0=diag0, what=f"{name}: ")
    print(f"{name}: warm-up marginals pose={e_w['pose']:.2e} landmarks={e_w['landmarks']:.2e}; final {pb.fmt(err)}")


# ----------------------------------------------------------------------------------------------------------------------
# D. chained revisits at benchmark sizes
# ----------------------------------------------------------------------------------------------------------------------
def test_chained_revisits_n2000(sd, oracle):
    """300 steps at N = 2000 x 1, one run_stream, defaults: every cadence's chained block holds rows the previous
    cadence updated (2 per step), rows of its own cadence (1 per step) and rows of 200 steps ago (1 per step).  Against
    the oracle piece by piece, and against the same stream with every solve behind its pass (`lookahead=0`)."""
    N = 2000
    s = scheduled_stream(N, revisit_schedule())
    n, steps = 3 + 2 * N, len(s[2])
    res = {}
    for mode, opts in (("chain", ()), ("plain", (("lookahead", 0),))):
        with sd.EkfSlam(n) as f:
            for k, v in opts:
                f.set_option(k, v)
            f.set_state_diag(s[0], s[1])
            f.run_stream(*s[2:])
            cad = f.cadence_counters()
            res[mode] = f.state() + (counters(sd, f).chained, f.flags(), f.last_pass())
        assert res[mode][3] == 0, mode
        assert cad == (steps * M // 40, steps), (mode, cad)
    print(f"\nrevisits N=2000: pass {res['chain'][4]}, chained {res['chain'][2]}")
    assert res["chain"][2] == steps * M // 40 - 1 and res["plain"][2] == 0
    obs = pb.observed_landmarks(s[4])
    mu, P = res["chain"][:2]
    e_path = pb.assert_filter_close(mu, P, *res["plain"][:2], obs, mean0=s[0], diag0=s[1], tol=PATH_TOL,
                                    corr_tol=pb.PATH_CORR_TOL, what="chain vs plain: ")
    assert orc.rel_fro(mu, res["plain"][0]) < PATH_TOL and orc.rel_fro(P, res["plain"][1]) < PATH_TOL
    om, oP = oracle["revisits_n2000"].result()
    err = pb.assert_filter_close(mu, P, om, oP, obs, mean0=s[0], diag0=s[1], what="chain vs oracle: ")
    print(f"revisits N=2000: oracle {pb.fmt(err)}; plain {pb.fmt(e_path)}")


def test_chained_scattered_n8000(sd, oracle):
    """40 steps at N = 8000 x 1, active bound off, the indices scattered over the whole state: both column panels of the
    chained row-slab pass carry updates.  Against the oracle on the observed and pose rows (downloaded alone), the diagonal
    and the row sums; the rows of landmarks never observed exactly as they started."""
    N = 8000
    s = scheduled_stream(N, scattered_schedule())
    n, steps = 3 + 2 * N, len(s[2])
    obs = pb.observed_landmarks(s[4])
    act = np.concatenate([np.arange(3), pb.landmark_rows(obs)])
    with sd.EkfSlam(n) as f:
        f.set_option("active_bound", 0)
        f.set_state_diag(s[0], s[1])
        f.run_stream(*s[2:])
        cad = f.cadence_counters()
        n_chained, kernel = counters(sd, f).chained, f.last_pass()
        rows = np.concatenate([f.covariance_block(0, 0, 3, n)] + [f.covariance_block(3 + 2 * int(j), 0, 2, n) for j in obs])
        assert f.flags() == 0
        mu, P = f.state()
    print(f"\nscattered N=8000: pass {kernel}, chained {n_chained}, cadences {cad}")
    assert cad == (steps * M // 40, steps) and n_chained == steps * M // 40 - 1
    assert kernel == "ekf::k_flush_rs<20, true, true, false>"
    ref = oracle["scattered_n8000"].result()
    assert np.array_equal(rows, P[act])                                   # the block download is the state's rows
    rest = np.setdiff1d(np.arange(n), act)
    assert not rows[:, rest].any()                                        # never correlated with unobserved landmarks
    for what, a, b in (("observed and pose rows", rows, ref["rows"]), ("diagonal", np.diag(P), ref["diag"]),
                       ("row sums", P.sum(axis=1), ref["rowsum"]), ("mean", mu, ref["mean"])):
        r = orc.rel_fro(a, b)
        assert r < TIGHT, f"{what}: rel Frobenius {r:.3e}"
    assert np.array_equal(mu[rest[rest >= 3]], s[0][rest[rest >= 3]])
    assert np.array_equal(np.diag(P)[rest], s[1][rest])
    err = pb.active_errors(mu[act], rows[:, act], ref["mean"][act], ref["rows"][:, act])
    pb.check_errors(err, TIGHT, "scattered N=8000: ")
    pb.assert_symmetric(rows[:, act], TIGHT)
    print(f"scattered N=8000: {pb.fmt(err)}")


# ----------------------------------------------------------------------------------------------------------------------
# E. chained handles side by side
# ----------------------------------------------------------------------------------------------------------------------
def test_two_chained_handles_from_two_host_threads(sd):
    """Two single-trajectory handles at N = 500 (each run_stream of 60 steps chained: 12 cadences, 11 chained solves), driven
    from two host threads at once: each comes out bit for bit as when it runs alone."""
    import slam_duckietown_amd.synthetic as syn
    N, steps = 500, 60
    streams = [syn.synthetic_stream(N, steps, M, 110 + t) for t in range(2)]
    n = 3 + 2 * N

    def run(st, out, slot, barrier=None):
        with sd.EkfSlam(n) as f:
            f.set_state_diag(st[0], st[1])
            f.stream_upload(*st[2:])
            if barrier is not None:
                barrier.wait()
            f.stream_run(0, steps)
            out[slot] = f.state() + (f.flags(), counters(sd, f).chained)

    alone, together = [None, None], [None, None]
    for t in range(2):
        run(streams[t], alone, t)
    barrier = threading.Barrier(2)
    threads = [threading.Thread(target=run, args=(streams[t], together, t, barrier)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
        assert not th.is_alive()
    for t in range(2):
        for out in (alone, together):
            assert out[t] is not None and out[t][2] == 0 and out[t][3] == steps * M // 40 - 1, (t, out[t][2:])
        assert np.array_equal(alone[t][0], together[t][0]) and np.array_equal(alone[t][1], together[t][1]), t
    s = streams[0]
    om, oP = _run_oracle(s[0].copy(), np.diag(s[1]), s, 0, steps)
    pb.assert_filter_close(*together[0][:2], om, oP, pb.observed_landmarks(s[4]), mean0=s[0], diag0=s[1])
