"""NumPy reference of the linear motion update (ekf_predict_linear), and the input sets the GPU tests use.

A prediction is (pose, F, Q): the NEW pose mean, taken verbatim, F = d(new pose)/d(old pose) (3 x 3) and the process noise Q
(3 x 3, its upper triangle is authoritative, positive SEMI-definite).  With G = blockdiag(F, I):  mean[0:3] = pose,
P <- G P G^T + Q  (Q embedded in the pose block).  Two formulations: the dense product, and the delta form on the deferred
representation P = P_base + W V + diag(dacc) that the kernel uses."""
import numpy as np

from oracle import ekf_oracle as orc
from tests import direct_model as dm


def sym_upper(Q):
    Qu = np.triu(np.asarray(Q, dtype=float))
    return Qu + np.triu(Qu, 1).T


def predict_linear(mean, cov, pose, F, Q):
    """The dense form: G P G^T with G = blockdiag(F, I), plus Q embedded."""
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    n = len(mean)
    G = np.eye(n)
    G[:3, :3] = np.asarray(F, dtype=float)
    out = G @ cov @ G.T
    out[:3, :3] += sym_upper(Q)
    mean[:3] = np.asarray(pose, dtype=float)
    return mean, out


def materialize(Pb_upper, W=None, V=None, dacc=None):
    """The covariance a deferred representation stands for: the upper triangle of P_base + W V + diag(dacc) (dacc on the pose
    diagonal), mirrored.  Nothing below the diagonal of Pb_upper is read.  W None: P_base alone."""
    U = np.triu(np.where(np.tri(len(Pb_upper), k=-1, dtype=bool), 0.0, Pb_upper))
    if W is not None:
        U = U + np.triu(W @ V)
        U[[0, 1, 2], [0, 1, 2]] += np.asarray(dacc, dtype=float)
    return U + np.triu(U, 1).T


def predict_linear_deferred(Pb_upper, W, V, dacc, F, Q):
    """The delta form, the algebra of k_predict_pose.  Pb_upper: P_base with NaN below the diagonal (never read); W (n x kb),
    V (kb x n), dacc (3): what is pending (W None: nothing).  Returns the new P_base (NaN below the diagonal still): with ranks
    pending (F - I) x is ADDED to rows 0..2 of P_base, x = P(0..2, j) the current column, and (F P_rr F^T + Q) - P_rr to the pose
    block; with nothing pending F x and F P_rr F^T + Q are written directly.  W, V and dacc are not touched."""
    Pb = np.array(Pb_upper, dtype=float)
    F, Qs = np.asarray(F, dtype=float), sym_upper(Q)
    iu = np.triu_indices(3)
    if W is None:
        x = Pb[:3, 3:]
        blk = np.triu(Pb[:3, :3])
        blk = blk + np.triu(blk, 1).T
        Pb[:3, 3:] = F @ x
        Pb[:3, :3][iu] = (F @ blk @ F.T + Qs)[iu]
        return Pb
    x = Pb[:3, 3:] + W[:3, :] @ V[:, 3:]
    cur = np.triu(Pb[:3, :3]) + np.triu(W[:3, :] @ V[:, :3]) + np.diag(np.asarray(dacc, dtype=float))
    cur = cur + np.triu(cur, 1).T
    Pb[:3, 3:] += (F - np.eye(3)) @ x
    Pb[:3, :3][iu] += ((F @ cur @ F.T + Qs) - cur)[iu]
    return Pb


def compose(pose, delta):
    """pose (+) delta: the increment delta = (dx, dy, dtheta) is given in the robot frame of pose = (x, y, theta); theta wrapped
    to [-pi, pi) (evaluation.wrap_angle's convention).  Returns (new pose, d(new)/d(pose), d(new)/d(delta))."""
    x, y, th = (float(v) for v in pose)
    dx, dy, dth = (float(v) for v in delta)
    c, s = np.cos(th), np.sin(th)
    new = np.array([x + c * dx - s * dy, y + s * dx + c * dy, (th + dth + np.pi) % (2 * np.pi) - np.pi])
    Fp = np.array([[1.0, 0.0, -s * dx - c * dy], [0.0, 1.0, c * dx - s * dy], [0.0, 0.0, 1.0]])
    Fd = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return new, Fp, Fd


# ---- a deferred representation of a given covariance (tests/test_predict_linear_cpu.py) ----
def defer(cov, kb, seed):
    """`cov` as the filter holds it kb ranks BEFORE a block update of kb random rows has been applied: P_base = cov (NaN below the
    diagonal), V = A cov, W = -(S^-1 V)^T with S = A cov A^T + R, plus a pending pose noise.  materialize() of the result is a
    genuine posterior: the pending product is as large against P_base as a real one."""
    n = len(cov)
    Pb = np.where(np.tri(n, k=-1, dtype=bool), np.nan, cov)
    if kb == 0:
        return Pb, None, None, None
    rng = np.random.default_rng(seed)
    A = np.zeros((kb, n))
    for k in range(kb):                                      # a row reads the pose and one landmark, like an observation
        l = int(rng.integers(0, (n - 3) // 2))
        A[k, :3] = rng.normal(size=3)
        A[k, 3 + 2 * l:5 + 2 * l] = rng.normal(size=2)
    V = A @ cov
    S = V @ A.T + np.eye(kb) * 0.05
    W = -np.linalg.solve(S, V).T
    return Pb, W, V, rng.uniform(0.0, 0.02, 3)


# ---- the input sets of tests/test_gpu_predict_linear.py (tests/test_predict_linear_cpu.py checks the two forms on them) ----
POSE_SHIFT = np.array([0.05, -0.03, 0.02])
KINDS = ("full", "rank1", "zero")


def draw(rng, mean, cov, kind="full"):
    """A prediction around the state (mean, cov): the pose moved by POSE_SHIFT, F = I + 0.3 randn, and Q = A A^T scaled to the
    pose block's size (trace / 3) -- A 3 x 3 (full rank), 3 x 1 (rank 1), or an all-zero Q."""
    pose = np.asarray(mean[:3], dtype=float) + POSE_SHIFT
    pose[2] = orc.wrap_pi(pose[2])
    F = np.eye(3) + 0.3 * rng.normal(size=(3, 3))
    scale = np.trace(np.asarray(cov)[:3, :3]) / 3.0
    if kind == "zero":
        Q = np.zeros((3, 3))
    else:
        A = rng.normal(size=(3, 3 if kind == "full" else 1))
        Q = A @ A.T
        Q *= scale / (np.trace(Q) / 3.0)
    return pose, F, Q


def case_small(seed=7, kind="full"):
    """Test 1: N = 20, 30 steps (dm.small_stream); the generator the prediction is drawn from at the state before the call."""
    return dm.small_stream(seed), np.random.default_rng(700 + seed + KINDS.index(kind))


BUILTIN = {"arc": (0.12, 0.3), "straight": (0.12, 0.004)}     # (lin, ang): |ang| above / below EkfConfig.arc_threshold


def builtin_inputs(mean, branch, cfg=None):
    """Test 2: the reference's own motion model as a linear prediction: (pose', G) of orc.motion_model and its noise."""
    cfg = cfg or orc.EkfConfig()
    lin, ang = BUILTIN[branch]
    pose, G = orc.motion_model(np.asarray(mean[:3], dtype=float), lin, ang, cfg)
    return lin, ang, pose, G, np.diag(cfg.motion_noise_diag())


BANK_APPLY = [1, 1, 0, 1]


def case_bank(seed=20):
    """Test 3: dm.case_bank's streams (N = 150 x 4) and the generator; trajectory 2 is not applied."""
    streams, _ = dm.case_bank(seed)
    return streams, np.random.default_rng(seed + 900)


CHAIN_N, CHAIN_PIECE, CHAIN_M = 500, 60, 8


def case_chain(seed=5, N=CHAIN_N):
    """Test 6: N = 500 x 1, two pieces of 60 stream steps of m = 8."""
    return orc.synthetic_stream(N, 2 * CHAIN_PIECE, CHAIN_M, seed), np.random.default_rng(seed + 950)


def slip_model(pose, u):
    """predict_custom's test model: a unicycle arc whose heading change is scaled by a slip factor that depends on the heading.
    u = (lin, ang, slip)."""
    lin, ang, slip = u
    x, y, th = pose
    da = ang * (1.0 + slip * np.sin(th))
    return np.array([x + lin * np.cos(th + 0.5 * da), y + lin * np.sin(th + 0.5 * da), th + da])


def slip_jacobian(pose, u):
    lin, ang, slip = u
    th = pose[2]
    da = ang * (1.0 + slip * np.sin(th))
    dda = ang * slip * np.cos(th)
    return np.array([[1.0, 0.0, -lin * np.sin(th + 0.5 * da) * (1.0 + 0.5 * dda)],
                     [0.0, 1.0, lin * np.cos(th + 0.5 * da) * (1.0 + 0.5 * dda)],
                     [0.0, 0.0, 1.0 + dda]])


SLIP_U = (0.15, 0.25, 0.2)
