"""The CPU model of the hypothesis bank's mixture row (k_hyp_mixture: ekf_hypotheses_mixture and ekf_hypotheses_run's log): a restatement of
`evaluation.mixture_pose` and of tests/resample_model.py's `weigh` in a chosen precision -- np.longdouble is the reference the GPU
test judges the device against, float64 is what tests/test_hyp_run_cpu.py holds within 1e-12 of it --, the judge both tests share
and the cases of the CPU test.  A plain module: nothing here needs a device.

The bar is the one tests/test_gpu_hyp_resample.py sets for the header's ess and logmean, restated here because no test module
imports another: rel(got, want) <= TOL = 1e-9, rel = |got - want| / max(1, |want|).  The mean heading is compared on the circle:
-pi and +pi are the same heading, and which of the two atan2 returns hangs on the sign of a sum that is zero up to rounding."""
import typing

import numpy as np

NONFINITE = 1                                              # EKF_FLAG_NONFINITE
TOL = 1e-9


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b)) if np.isfinite(b) else (0.0 if a == b else np.inf)


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


class Mixture(typing.NamedTuple):
    mean: np.ndarray                                       # (3,)
    cov: np.ndarray                                        # (3, 3)
    ess: float
    evidence: float
    live: int
    best: int


def mixture(pose, blk, loglik, flags, dtype=np.longdouble, mutant=None):
    """The row of a bank (pose (K, 3), blk (K, 3, 3), loglik (K,), flags (K,)) in `dtype`.  `mutant`: one of the three wrong
    implementations the CPU test shows the judge to catch -- "nan" (multiplies a dead hypothesis by its zero weight instead of
    skipping it), "linear" (averages the heading as a number), "unwrapped" (does not wrap the heading's deviation)."""
    pose, blk, ll = np.asarray(pose, dtype=dtype), np.asarray(blk, dtype=dtype), np.asarray(loglik, dtype=dtype)
    K = len(ll)
    ok = np.isfinite(ll) & ((np.asarray(flags) & NONFINITE) == 0)
    w = np.zeros(K, dtype=dtype)
    if ok.any():
        top = ll[ok].max()
        w[ok] = np.exp(ll[ok] - top)
        # what weighs is float64's business, as in resample_model.weigh: a weight whose double exp underflows to 0 is dead
        w[ok] = np.where(np.exp((ll[ok] - top).astype(np.float64)) > 0.0, w[ok], 0)
    use = w > 0
    if not use.any():
        return Mixture(np.full(3, np.nan), np.full((3, 3), np.nan), 0.0, -np.inf, 0, -1)
    s, s2 = w.sum(), (w * w).sum()
    ess, evidence = s * s / s2, top + np.log(s / dtype(K))
    best = int(np.nonzero(use & (ll == top))[0][0])
    if mutant == "nan":
        p, P, wn = pose, blk, w / s
    else:
        p, P, wn = pose[use], blk[use], w[use] / s
    th = wn @ p[:, 2] if mutant == "linear" else np.arctan2(wn @ np.sin(p[:, 2]), wn @ np.cos(p[:, 2]))
    mean = np.array([wn @ p[:, 0], wn @ p[:, 1], th], dtype=dtype)
    d = p - mean
    if mutant != "unwrapped":
        d[:, 2] = (d[:, 2] + dtype(np.pi)) % (2 * dtype(np.pi)) - dtype(np.pi)
    cov = np.einsum("k,kij->ij", wn, P) + np.einsum("k,ki,kj->ij", wn, d, d)
    return Mixture(mean, (cov + cov.T) / 2, ess, evidence, int(use.sum()), best)


def gaps(got, want):
    """The largest rel() of mean, covariance, ess and evidence of `got` against the model's row `want` (both with something
    alive), the heading on the circle."""
    g = [rel(float(got.mean[i]), float(want.mean[i])) for i in range(2)]
    g.append(abs(float(wrap(float(got.mean[2]) - float(want.mean[2])))))
    g += [rel(float(a), float(b)) for a, b in zip(np.ravel(got.cov), np.ravel(want.cov))]
    g += [rel(float(got.ess), float(want.ess)), rel(float(got.evidence), float(want.evidence))]
    return max(g)


def judge(got, pose, blk, loglik, flags, tol=TOL):
    """What the tests ask of a row `got` (anything with mean, cov, ess, evidence, live, best) for the bank it was formed from:
    None, or what is wrong."""
    want = mixture(pose, blk, loglik, flags)
    if got.live != want.live or got.best != want.best:
        return f"live {got.live} best {got.best} where the model has {want.live} and {want.best}"
    if want.live == 0:
        if not (np.isnan(got.mean).all() and np.isnan(got.cov).all() and got.ess == 0.0 and got.evidence == -np.inf):
            return "a degenerate bank must give NaN, ess 0 and evidence -inf"
        return None
    if not (np.isfinite(np.asarray(got.mean, dtype=np.float64)).all() and np.isfinite(np.asarray(got.cov, dtype=np.float64)).all()):
        return "not finite: a dead hypothesis reached the sums"
    if not np.array_equal(got.cov, np.transpose(got.cov)):
        return "the covariance is not symmetric"
    g = gaps(got, want)
    return None if g <= tol else f"gap {g:.3e} above {tol:g}"


# ---- the cases of the CPU test; the GPU test builds the same six on the device -------------------------------------------------
CASES = ("spread", "uniform", "one-hot", "headings at +-pi", "a flagged hypothesis holding NaN", "degenerate")
EDGE = 0.1                                                 # the headings case: pi - EDGE and -pi + EDGE in equal weight


def cpu_case(name, K=65, seed=0):
    """(pose, blk, loglik, flags) of one of CASES."""
    rng = np.random.default_rng(seed + K)
    pose = np.column_stack([rng.normal(1.0, 0.5, K), rng.normal(-2.0, 0.5, K), rng.uniform(-np.pi, np.pi, K)])
    a = rng.normal(0.0, 0.1, (K, 3, 3))
    blk = a @ np.transpose(a, (0, 2, 1)) + 1e-3 * np.eye(3)
    ll, flags = rng.normal(-7.0, 2.0, K), np.zeros(K, dtype=np.uint32)
    if name == "uniform":
        ll[:] = -3.25
    elif name == "one-hot":
        ll[:] = -1e4
        ll[K // 3] = -2.0
    elif name == "headings at +-pi":
        ll[:] = -1.5
        pose[:, 2] = np.where(np.arange(K) % 2 == 0, np.pi - EDGE, -np.pi + EDGE)
        if K % 2 and K > 1:                                # (equal weight: an odd one out weighs nothing)
            ll[K - 1] = -np.inf
    elif name == "a flagged hypothesis holding NaN":
        k = K // 2
        flags[k], pose[k], blk[k], ll[k] = NONFINITE, np.nan, np.nan, ll.max() + 1.0
    elif name == "degenerate":
        flags[:] = NONFINITE
    return pose, blk, ll, flags
