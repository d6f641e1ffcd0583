"""What the GPU tests of the hypothesis bank's resampling need of a device: a mapped handle with forked slots, observations as a
mean sees them, a hypothesis against a forked slot bit for bit, and a whole bank downloaded into tests/resample_model.py's `Bank`.
A plain module (the fixtures come from tests/gpu_support.py)."""
import numpy as np

from oracle import ekf_oracle as orc
from tests import resample_model as rm
from tests import streams
from tests.gpu_support import pbase

SLAM_STEPS = 30


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def observe(mean, lms, rng=None, noise=0.01):
    """Ranges and bearings of the landmarks `lms` as the mean itself sees them, plus a little noise (none without `rng`)."""
    lms = np.asarray(lms, dtype=np.int64)
    d = np.asarray(mean)[3:].reshape(-1, 2)[lms] - np.asarray(mean)[:2]
    er = rng.normal(0.0, noise, len(lms)) if rng is not None else 0.0
    eb = rng.normal(0.0, noise, len(lms)) if rng is not None else 0.0
    return lms.astype(np.int32), np.hypot(d[:, 0], d[:, 1]) + er, wrap(np.arctan2(d[:, 1], d[:, 0]) - mean[2] + eb)


def mapped_handle(sd, B, N=20, seed=11):
    """A handle of B slots whose slot 0 holds an N-landmark map from 30 SLAM steps (dense cross-covariances), flushed, and every
    other slot a fork of it."""
    _, lin, ang, idx, zr, zb, m = streams.wandering(N, B, SLAM_STEPS, 8, seed)
    worlds = [orc.synthetic_world(N, seed + 1 + t) for t in range(B)]
    f = sd.EkfSlam(3 + 2 * N, batch=B)
    for b in range(B):
        f.set_state_diag(worlds[b][2], worlds[b][3], b)
    f.stream_upload(lin, ang, idx, zr, zb, m)
    f.stream_run(0, SLAM_STEPS)
    f.flush()
    if B > 1:
        f.fork(0)
    return f


def sparse_handle(sd, B, N, slam_lms, seed):
    """A handle of B slots at N landmarks on the general kernels: slot 0 mapped by one SLAM step per list of `slam_lms` (observed
    from its mean), flushed, every other slot a fork of it -- the large states, where 30 dense steps would take too long."""
    rng = np.random.default_rng(seed)
    world = orc.synthetic_world(N, seed)
    f = sd.EkfSlam(3 + 2 * N, batch=B)
    f.set_option("small_state", 0)
    for b in range(B):
        f.set_state_diag(world[2], world[3], b)
    none = [[]] * (B - 1)
    for lms in slam_lms:
        o = observe(f.mean(0), lms, rng)
        f.step(0.004, 0.02, [o[0]] + none, [o[1]] + none, [o[2]] + none)
    f.flush()
    if B > 1:
        f.fork(0)
    return f


def frozen_part(sd, f, b):
    """What a localisation call or an adopt must leave alone, raw: every stored P(a, b) with a, b >= 3 -- also below the diagonal
    and in the padding --, and the landmark means (tests/test_gpu_localize.py's)."""
    raw = pbase(sd, f, b)
    n_max = f.n_max
    if n_max <= 4096:
        ld = 64
        while ld < n_max:
            ld *= 2
        rows = raw.reshape(-1, ld)[3:].copy()
        rows[:, :3] = 0.0
    else:
        ld = (n_max + 63) // 64 * 64
        rows = raw.reshape(-1, ld, 4096)[:, 3:].copy()
        rows[0, :, :3] = 0.0
    return rows, f.mean(b)[3:].copy()


def frozen_same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def assert_same_bits(bank, k, f, b, what):
    """Hypothesis k against slot b: pose mean, pose block, P[0:3, :]."""
    n = f.size(b)
    pose, rows = f.mean(b)[:3].copy(), f.covariance_block(0, 0, 3, n, b)
    hp, hc = bank.poses()
    hr = bank.rows(k)
    assert np.isfinite(hp[k]).all() and np.isfinite(hr).all(), f"{what}: NaN"
    assert np.array_equal(hp[k], pose), f"{what}: pose mean {hp[k]} where the slot has {pose}"
    assert np.array_equal(hc[k], rows[:, :3]), f"{what}: pose block"
    assert np.array_equal(hr, rows), f"{what}: pose rows differ in {int((hr != rows).sum())} entries"


def snapshot(bank):
    """The whole bank as the model's `Bank`."""
    pose, cov, ll, nobs, nrej, fl = bank._download()
    return rm.Bank(pose, cov, np.stack([bank.rows(k) for k in range(bank.count)]), ll, nobs, nrej, fl)


def same_snapshot(a, b):
    return all(rm.bits_equal(getattr(a, name), getattr(b, name)) for name in ("pose", "blk", "rows", "loglik", "n_obs", "n_rej", "flags"))
