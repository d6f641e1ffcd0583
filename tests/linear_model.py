"""NumPy reference of the linear measurement update (ekf_update_linear), and the input sets the GPU tests use.

A measurement is (landmarks, H, R, r): the sub-state is [x, y, theta, l_j0 x, l_j0 y, ...] over `landmarks` in the order given
(EkfSlam.joint's), H is D x (3 + 2 k), R D x D (its upper triangle is authoritative) and r the measurement z (y = z - H mean[s],
no row wrapped) or, with innovation=True, the innovation y itself.  S = H P[s, s] H^T + R, K = P[:, s] H^T S^-1, mean += K y,
P -= K S K^T.  Returns (mean, cov, nis, dof, applied); a NIS above `gate` rejects the whole update (the inputs come back
unchanged)."""
import numpy as np

from oracle import ekf_oracle as orc
from tests import direct_model as dm


def sub_indices(landmarks):
    s = [0, 1, 2]
    for l in landmarks:
        s += [3 + 2 * int(l), 4 + 2 * int(l)]
    return np.array(s, dtype=np.int64)


def sym_upper(R):
    Ru = np.triu(np.asarray(R, dtype=float))
    return Ru + np.triu(Ru, 1).T


def full_H(n, landmarks, H):
    H = np.asarray(H, dtype=float)
    Hf = np.zeros((H.shape[0], n))
    Hf[:, sub_indices(landmarks)] = H
    return Hf


def linear_update(mean, cov, landmarks, H, R, r, innovation=False, gate=np.inf):
    """The simple form."""
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    r = np.asarray(r, dtype=float).reshape(-1)
    if len(r) == 0:
        return mean, cov, 0.0, 0, False
    Hf, RR = full_H(len(mean), landmarks, H), sym_upper(R)
    y = r if innovation else r - Hf @ mean
    U = Hf @ cov
    S = U @ Hf.T + RR
    nis = float(y @ np.linalg.solve(S, y))
    if not nis <= gate:
        return mean, cov, nis, len(r), False
    return mean + U.T @ np.linalg.solve(S, y), cov - U.T @ np.linalg.solve(S, U), nis, len(r), True


def linear_update_joseph(mean, cov, landmarks, H, R, r, innovation=False, gate=np.inf):
    """The Joseph form (I - K H) P (I - K H)^T + K R K^T."""
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    r = np.asarray(r, dtype=float).reshape(-1)
    if len(r) == 0:
        return mean, cov, 0.0, 0, False
    n = len(mean)
    Hf, RR = full_H(n, landmarks, H), sym_upper(R)
    y = r if innovation else r - Hf @ mean
    S = Hf @ cov @ Hf.T + RR
    K = np.linalg.solve(S, Hf @ cov).T
    nis = float(y @ np.linalg.solve(S, y))
    if not nis <= gate:
        return mean, cov, nis, len(r), False
    A = np.eye(n) - K @ Hf
    return mean + K @ y, A @ cov @ A.T + K @ RR @ K.T, nis, len(r), True


# ---- the input sets of tests/test_gpu_linear.py (tests/test_linear_cpu.py checks that the two forms agree on them) ----
def dense_noise(rng, D):
    """A dense D x D noise covariance on the scale of the project's noise: sigma 0.02 - 0.1, correlated, positive definite
    by construction (a Gram matrix plus the identity, scaled to unit diagonal)."""
    sig = rng.uniform(0.02, 0.1, D)
    A = rng.normal(size=(D, D))
    C = A @ A.T / D + np.eye(D)
    dg = np.sqrt(np.diag(C))
    C = C / dg[:, None] / dg[None, :]
    return sig[:, None] * C * sig[None, :]


def dense_rows(rng, mean, cov, landmarks, D, offset_sigmas=1.0):
    """A dense D-row measurement of the sub-state drawn around the filter's own belief: H uniform in [-1, 1], dense R,
    z = H mean[s] + offset_sigmas * sqrt(diag S) * N(0, 1)."""
    s = sub_indices(landmarks)
    H = rng.uniform(-1.0, 1.0, (D, len(s)))
    R = dense_noise(rng, D)
    S = H @ cov[np.ix_(s, s)] @ H.T + R
    z = H @ mean[s] + offset_sigmas * np.sqrt(np.diag(S)) * rng.normal(size=D)
    return H, R, z


SMALL_LANDMARKS = [5, 11, 2]       # (in no order; all observed)


def case_small(seed=7):
    """Test 1: N = 20, 30 steps (dm.small_stream), then a dense H with D = 7 over the pose and three observed landmarks, in
    z mode (never-observed landmarks in a dense H: case_bank)."""
    s = dm.small_stream(seed)
    om, oP = dm.dense_of(s, dm.SMALL_STEPS)
    rng = np.random.default_rng(400 + seed)
    H, R, z = dense_rows(rng, om, oP, SMALL_LANDMARKS, 7)
    return s, SMALL_LANDMARKS, H, R, z


def range_bearing(xs):
    """The built-in observation model of one landmark on the sub-state [x, y, theta, lx, ly] (oracle/ekf_oracle.py's):
    h = (range, bearing) and its 2 x 5 Jacobian."""
    dx, dy = xs[3] - xs[0], xs[4] - xs[1]
    q = dx * dx + dy * dy
    sq = np.sqrt(q)
    h = np.array([sq, np.arctan2(dy, dx) - xs[2]])
    J = np.array([[-sq * dx, -sq * dy, 0.0, sq * dx, sq * dy], [dy, -dx, -q, -dy, dx]]) / q
    return h, J


HOOK_LANDMARK = 9


def case_hook(seed=7):
    """Test 2: the stream of case_small and one observation (range, bearing) of landmark 9 near the oracle's belief."""
    s = dm.small_stream(seed)
    om, _ = dm.dense_of(s, dm.SMALL_STEPS)
    h, _ = range_bearing(om[[0, 1, 2, 3 + 2 * HOOK_LANDMARK, 4 + 2 * HOOK_LANDMARK]])
    return s, HOOK_LANDMARK, float(h[0] + 0.05), float(orc.wrap_pi(h[1] - 0.03))


def selection_of(targets, z, R):
    """A direct update (dm's fixes) as a linear one: landmarks, the selection H, block-diagonal R and z."""
    lms = [int(t) for t in targets if t >= 0]
    s = list(sub_indices(lms))
    rows = dm.rows_of(targets)
    H = np.zeros((len(rows), len(s)))
    for a, x in enumerate(rows):
        H[a, s.index(int(x))] = 1.0
    zz, RR, o = np.zeros(len(rows)), np.zeros((len(rows), len(rows))), 0
    for t, zi, Ri in zip(targets, z, R):
        d = 3 if t == dm.POSE else 2
        zz[o:o + d] = np.asarray(zi, dtype=float)[:d]
        RR[o:o + d, o:o + d] = sym_upper(np.asarray(Ri, dtype=float)[:d, :d])
        o += d
    return lms, H, RR, zz


def case_selection(seed=7):
    """Test 3: dm.case_small's fixes without the pose's theta row wrapped -- a position fix and two landmark fixes, one on a
    never-observed landmark -- as a selection H with block-diagonal R."""
    s, t, z, R = dm.case_small(seed)
    t = [dm.POSITION] + t[1:]
    return s, t, z, R


BANK_NEVER = (130, 149)


def case_bank(seed=20):
    """Test 4: dm.case_bank's streams (N = 150 x 4, landmarks 0 .. 119 observed, 120 .. 149 never).  Per trajectory
    (landmarks, H, R) and how the innovation is made from the pre-call state (bank_innovation): 0 a pose-only heading row;
    1 D = 32 over 16 landmarks, two of them never observed; 2 nothing; 3 a constraint between two landmarks 10 sigma off."""
    streams, _ = dm.case_bank(seed)
    rng = np.random.default_rng(seed + 500)
    lm1 = [int(j) for j in rng.permutation(118)[:14]]
    lm1 = lm1[:5] + [BANK_NEVER[1]] + lm1[5:11] + [BANK_NEVER[0]] + lm1[11:]
    H1 = rng.uniform(-1.0, 1.0, (32, 35))
    Hc = np.zeros((2, 7))
    Hc[0, 5], Hc[1, 6], Hc[0, 3], Hc[1, 4] = 1.0, 1.0, -1.0, -1.0
    meas = [([], np.array([[0.0, 0.0, 1.0]]), np.array([[0.03 ** 2]])),
            (lm1, H1, dense_noise(rng, 32)),
            ([], np.zeros((0, 3)), np.zeros((0, 0))),
            ([40, 7], Hc, dense_noise(rng, 2))]
    return streams, meas, rng.normal(size=32)


def bank_innovation(b, meas, draw, mean, cov):
    """The innovation trajectory b of case_bank brings, from its state (mean, cov) just before the call: for trajectory 0 one
    sigma of S around zero (`draw`: fixed standard normal values), for trajectory 3 ten sigma on both rows, for trajectory 1 a
    tenth of a sigma, a never-observed landmark counting with variance 0.01.  (The mean update of a never-observed landmark
    tied into a dense H is a sum of terms landmark_init_var * H * S^-1 y that cancel: at one sigma of the full S the two
    NumPy forms themselves differ by 4e-11 in the mean, at one sigma of this S by 2e-11 -- above the 1e-11 they are held to.)"""
    lms, H, R = meas[b]
    if H.shape[0] == 0:
        return np.zeros(0)
    s = sub_indices(lms)
    Ps = cov[np.ix_(s, s)]
    sd = np.sqrt(np.diag(H @ np.where(Ps > 1.0, 0.01, Ps) @ H.T + sym_upper(R)))
    return 10.0 * sd if b == 3 else (0.1 if b == 1 else 1.0) * sd * draw[:len(sd)]


def bank_follow_up(b):
    """The landmarks the ten steps after the call observe: for trajectory 1 the two formerly unobserved ones of its sub-state
    (the check of the bound rise), for the others one observed and one never-observed landmark of their (smaller) maps."""
    return list(BANK_NEVER) if b == 1 else [3, 140]


def follow_up_obs(mean, idx, k):
    """Observations of `idx` consistent with `mean` to a few centimetres / hundredths of a radian (step k's offsets)."""
    zr, zb = [], []
    for a, l in enumerate(idx):
        h, _ = range_bearing(mean[[0, 1, 2, 3 + 2 * l, 4 + 2 * l]])
        zr.append(float(h[0] + 0.02 * np.cos(k + a)))
        zb.append(float(orc.wrap_pi(h[1] + 0.01 * np.sin(2 * k + a))))
    return zr, zb


CONSTRAINT_PAIR = (3, 12)
CONSTRAINT_SIGMA = 1e-3


def case_constraint(seed=7):
    """Test 5: the stream of case_small; landmark 12 lies `offset` from landmark 3 -- the oracle's own separation moved by
    (0.05, -0.04) m -- with sigma 1 mm per axis, far below the map's relative uncertainty."""
    s = dm.small_stream(seed)
    om, _ = dm.dense_of(s, dm.SMALL_STEPS)
    i, j = CONSTRAINT_PAIR
    offset = om[3 + 2 * j:5 + 2 * j] - om[3 + 2 * i:5 + 2 * i] + np.array([0.05, -0.04])
    return s, i, j, offset, np.eye(2) * CONSTRAINT_SIGMA ** 2


def constraint_rows(i, j, offset, cov):
    """What EkfSlam.constrain_landmarks(i, j, offset, cov) hands to update_linear: landmarks sorted, l_j - l_i = offset."""
    lms = sorted([int(i), int(j)])
    H = np.zeros((2, 7))
    for a in range(2):
        H[a, 3 + 2 * lms.index(int(j)) + a] = 1.0
        H[a, 3 + 2 * lms.index(int(i)) + a] = -1.0
    return lms, H, np.asarray(cov, dtype=float), np.asarray(offset, dtype=float)


PANEL_N, PANEL_STEPS, PANEL_HIGH, PANEL_LOW = 2050, 5, 2046, 3


def case_panel(seed=3, N=PANEL_N, high=PANEL_HIGH):
    """Test 6: N = 2050 (n = 4103: two column panels), diagonal start, 5 steps of m = 8, then a constraint between the
    never-observed landmark 2046 -- state indices 4095 and 4096, the pair that straddles the panel -- and the first landmark
    the stream observes (N and the high landmark scale down for the CPU check of the two forms)."""
    s = orc.synthetic_stream(N, PANEL_STEPS, 8, seed)
    low = int(np.asarray(s[4]).ravel()[0])
    offset = s[0][3 + 2 * high:5 + 2 * high] - s[0][3 + 2 * low:5 + 2 * low] + np.array([0.1, -0.2])
    return s, low, high, offset, np.eye(2) * 0.05 ** 2


def distance_model(xs):
    """update_custom's test model on the sub-state [pose, l_a, l_b]: the distance between the two landmarks, its analytic
    Jacobian, and a bound on its third derivatives (of |d| by d: at most 3 / |d|^2)."""
    d = xs[5:7] - xs[3:5]
    r = float(np.hypot(d[0], d[1]))
    J = np.zeros((1, 7))
    J[0, 5:7], J[0, 3:5] = d / r, -d / r
    return np.array([r]), J, 3.0 / (r * r)


CUSTOM_PAIR = (4, 10)


def case_custom(seed=7):
    """The update_custom case: the stream of case_small, a tape measure between landmarks 4 and 10 reading the oracle's
    distance plus 3 cm, sigma 2 cm."""
    s = dm.small_stream(seed)
    om, _ = dm.dense_of(s, dm.SMALL_STEPS)
    h, _, _ = distance_model(om[sub_indices(CUSTOM_PAIR)])
    return s, list(CUSTOM_PAIR), np.array([h[0] + 0.03]), np.array([[0.02 ** 2]])
