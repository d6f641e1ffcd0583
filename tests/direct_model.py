"""NumPy reference of the direct measurement update (ekf_update_direct), and the input sets the GPU tests use.

A fix is (target, z, R): target -1 = pose (x, y, theta), -2 = position (x, y), l >= 0 = landmark l's (x, y).  The rows of all
fixes are stacked in the order given, R block-diagonal:  y = z - mean[s] (theta wrapped to [-pi, pi)),  S = P[s, s] + R,
K = P[:, s] S^-1,  mean += K y,  P -= K S K^T.  Returns (mean, cov, nis, dof, applied); a NIS above `gate` rejects the whole
update (the inputs come back unchanged)."""
import numpy as np

from oracle import ekf_oracle as orc

POSE, POSITION = -1, -2


def rows_of(targets):
    s = []
    for t in targets:
        s += [0, 1, 2] if t == POSE else [0, 1] if t == POSITION else [3 + 2 * int(t), 4 + 2 * int(t)]
    return np.array(s, dtype=np.int64)


def stack(mean, targets, z, R):
    s = rows_of(targets)
    D = len(s)
    zz, RR, o = np.zeros(D), np.zeros((D, D)), 0
    for t, zi, Ri in zip(targets, z, R):
        d = 3 if t == POSE else 2
        zz[o:o + d] = np.asarray(zi, dtype=float)[:d]
        Ru = np.triu(np.asarray(Ri, dtype=float)[:d, :d])          # the upper triangle is authoritative
        RR[o:o + d, o:o + d] = Ru + np.triu(Ru, 1).T
        o += d
    y = zz - mean[s]
    y[s == 2] = orc.wrap_pi(y[s == 2])
    return s, y, RR


def direct_update(mean, cov, targets, z, R, gate=np.inf):
    """The simple form."""
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    if len(targets) == 0:
        return mean, cov, 0.0, 0, False
    s, y, RR = stack(mean, targets, z, R)
    S = cov[np.ix_(s, s)] + RR
    U = cov[s, :]
    nis = float(y @ np.linalg.solve(S, y))
    if not nis <= gate:
        return mean, cov, nis, len(s), False
    SiU = np.linalg.solve(S, U)
    return mean + U.T @ np.linalg.solve(S, y), cov - U.T @ SiU, nis, len(s), True


def direct_update_joseph(mean, cov, targets, z, R, gate=np.inf):
    """The Joseph form (I - K H) P (I - K H)^T + K R K^T."""
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    if len(targets) == 0:
        return mean, cov, 0.0, 0, False
    s, y, RR = stack(mean, targets, z, R)
    n = len(mean)
    H = np.zeros((len(s), n))
    H[np.arange(len(s)), s] = 1.0
    S = H @ cov @ H.T + RR
    K = np.linalg.solve(S, H @ cov).T
    nis = float(y @ np.linalg.solve(S, y))
    if not nis <= gate:
        return mean, cov, nis, len(s), False
    A = np.eye(n) - K @ H
    return mean + K @ y, A @ cov @ A.T + K @ RR @ K.T, nis, len(s), True


def direct_update_sequential(mean, cov, targets, z, R):
    """One fix per update, in the order given (no gate: the gate is a property of the joint update)."""
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    for t, zi, Ri in zip(targets, z, R):
        mean, cov, _, _, _ = direct_update(mean, cov, [t], [zi], [Ri])
    return mean, cov


# ---- the input sets of tests/test_gpu_direct.py (tests/test_direct_cpu.py checks that the three forms agree on them) ----
def noise_block(rng, d):
    """A fix's noise covariance on the scale of the project's noise: sigma 0.02 - 0.1 m, 0.02 - 0.05 rad, correlated."""
    sig = np.concatenate([rng.uniform(0.02, 0.1, 2), rng.uniform(0.02, 0.05, 1)])[:d]
    A = rng.uniform(-0.4, 0.4, (d, d))
    C = np.eye(d) + np.triu(A, 1) + np.triu(A, 1).T
    return sig[:, None] * C * sig[None, :]


def make_fixes(rng, mean, cov, targets, offset_sigmas=1.0):
    """Measurements of `targets` drawn around the filter's own belief: z = mean[s] + offset_sigmas * sqrt(diag S) * N(0, 1)."""
    z, R = [], []
    for t in targets:
        d = 3 if t == POSE else 2
        s = rows_of([t])
        Rb = noise_block(rng, d)
        sd = np.sqrt(np.diag(cov)[s] + np.diag(Rb))
        zi = np.zeros(3)
        zi[:d] = mean[s] + offset_sigmas * sd * rng.normal(size=d)
        Rf = np.zeros((3, 3))
        Rf[:d, :d] = Rb
        z.append(zi)
        R.append(Rf)
    return z, R


def run_dense(N, steps, m, seed):
    """The dense oracle's state after `steps` steps of synthetic_stream(N, steps, m, seed), and the stream."""
    s = orc.synthetic_stream(N, steps, m, seed)
    cfg = orc.EkfConfig()
    om, oP = s[0].copy(), np.diag(s[1])
    for k in range(steps):
        om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
    return s, om, (oP + oP.T) / 2


def observed(stream):
    return np.unique(np.asarray(stream[4]).ravel())


def dense_of(s, steps):
    """The dense oracle's state after the first `steps` steps of the stream `s`."""
    cfg = orc.EkfConfig()
    om, oP = s[0].copy(), np.diag(s[1])
    for k in range(steps):
        om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
    return om, (oP + oP.T) / 2


SMALL_STEPS = 30


def small_stream(seed=7):
    """N = 20: 31 steps of m = 4 over the landmarks 0 .. 15 (synthetic_stream(16, ...)), the state extended by the landmarks
    16 .. 19, which are never observed (prior variance landmark_init_var)."""
    s = orc.synthetic_stream(16, SMALL_STEPS + 1, 4, seed)
    rng = np.random.default_rng(300 + seed)
    mean0 = np.concatenate([s[0], rng.uniform(-1.0, 1.0, 8)])
    diag0 = np.concatenate([s[1], np.full(8, orc.EkfConfig().landmark_init_var)])
    return (mean0, diag0) + tuple(s[2:])


def case_small(seed=7):
    """Test 1: N = 20, 30 steps of m = 4 (landmarks 16 .. 19 never observed): a pose fix plus two landmark fixes, one of
    them on the never-observed landmark 17."""
    s = small_stream(seed)
    om, oP = dense_of(s, SMALL_STEPS)
    rng = np.random.default_rng(100 + seed)
    targets = [POSE, 5, 17]
    z, R = make_fixes(rng, om, oP, targets[:2])
    z1, R1 = make_fixes(rng, om, np.diag(np.full(len(om), 0.01)), [17])   # (a survey within decimetres of the prior mean)
    return s, targets, z + z1, R + R1


def case_bank(seed=20):
    """Test 2: N = 150 x 4, 30 steps of m = 4 (landmarks 0 .. 119 observed, 120 .. 149 never).  Trajectory 0: pose only;
    1: position plus 15 landmarks, two of them never observed (D = 32); 2: nothing; 3: a pose fix 10 sigma off."""
    streams, fixes = [], []
    rng = np.random.default_rng(seed)
    for b in range(4):
        s, om, oP = run_dense(150, 30, 4, seed + b)
        streams.append(s)
        if b == 0:
            t = [POSE]
        elif b == 1:
            t = [POSITION] + [int(j) for j in rng.permutation(118)[:13]] + [130, 149]
            t = t[:3] + [t[-1]] + t[3:-1]                       # (a never-observed one in the middle of the list)
        elif b == 2:
            t = []
        else:
            t = [POSE]
        z, R = make_fixes(rng, om, oP, t, offset_sigmas=1.0)
        if b == 3:
            sd = np.sqrt(np.diag(oP)[:3] + np.diag(R[0]))
            z[0][:3] = om[:3] + 10.0 * sd
        fixes.append((t, z, R))
    return streams, fixes


def case_large(seed=3):
    """Test 3: N = 2060 (n = 4123, beyond one column panel), 40 steps of m = 8 (landmarks 0 .. 319) and one more step that
    observes landmark 2059: a pose fix, landmark 0, landmark 2059 and the never-observed landmark 1000."""
    N, steps = 2060, 40
    s = orc.synthetic_stream(N, steps, 8, seed)
    return s, [POSE, 0, 2059, 1000]


def case_three(seed=11):
    """Test 4: N = 150, three fixes."""
    s, om, oP = run_dense(150, 30, 4, seed)
    rng = np.random.default_rng(200 + seed)
    targets = [POSE, 3, 77]
    z, R = make_fixes(rng, om, oP, targets)
    return s, targets, z, R


GAUGE_N, GAUGE_STEPS, GAUGE_M, GAUGE_SEED = 60, 40, 4, 5
GAUGE_ANCHORS = (2, 31)
GAUGE_SIGMA = 0.01


def gauge_config():
    """A filter whose relative map is tight against its gauge: measurement sigma 0.08 (the stream's noise is 0.01 m) under
    the default pose prior of variance 0.1 -- the map is known to centimetres, its place in the world to 0.35 m.  On the
    dense oracle the anchored landmarks then lie at most 4.6 sigma from the survey, the unanchored ones at least 7.2."""
    return dict(meas_sigma=0.08)


def case_gauge():
    """Test 6: the stream, the survey = a rigid transform (rotation 0.02 rad about the origin, translation (2.5, -1.5): nine
    sigma of the prior gauge) of the true landmark positions, and the two anchors."""
    s = orc.synthetic_stream(GAUGE_N, GAUGE_STEPS, GAUGE_M, GAUGE_SEED)
    _, lm, _, _ = orc.synthetic_world(GAUGE_N, GAUGE_SEED)
    c, si = np.cos(0.02), np.sin(0.02)
    survey = lm @ np.array([[c, si], [-si, c]]) + np.array([2.5, -1.5])
    return s, survey


def within_sigmas(mean, blocks, survey, which, k=5.0):
    """Per landmark of `which`: the Mahalanobis distance of its estimate from the survey under its 2 x 2 marginal is <= k."""
    out = []
    for j in which:
        d = mean[3 + 2 * j:5 + 2 * j] - survey[j]
        out.append(float(d @ np.linalg.solve(blocks[j], d)) <= k * k)
    return np.array(out)
