"""The definition of a change of frame (EkfSlam.transform, ekf_transform; k_transform in csrc/ekf_transform.hip), in NumPy.

A rigid frame T = (t, phi) -- the old frame expressed in the new one -- with covariance Sigma (None: known exactly) maps every
item of the state x = [pose; landmarks].  With R = rot(phi), J2 = [[0, -1], [1, 0]]:

    landmark  l' = t + R l                      A_l = [I2 | J2 R l]                B_l = R
    pose      p' = (t + R p_xy, theta + phi)    A_p = [[I2, J2 R p_xy], [0 0 1]]   B_p = diag(R, 1)      (theta is not wrapped)
    P' = J P J^T + A Sigma A^T,    J = blockdiag(B_p, R, R, ...),    A = [A_p; A_l0; A_l1; ...]  (n x 3)

``transform_dense`` applies J blockwise (n = 4099 takes well under a second) and also returns the entrywise bounds the tests
scale their tolerances by: |J| |P| |J|^T + |A| |Sigma| |A|^T for the covariance, |t| + |R| |l| (|theta| + |phi|) for the mean."""
import numpy as np

from tests.join_model import rot  # noqa: F401  (the one definition of R = rot(phi); nothing else is shared with that model)

J2 = np.array([[0.0, -1.0], [1.0, 0.0]])


def _congruence(P, R):
    """blockdiag(diag(R, 1), R, R, ...) P blockdiag(...)^T, block by block."""
    n = P.shape[0]
    N = (n - 3) // 2
    Y = P.copy()
    Y[:2, :] = R @ P[:2, :]
    if N:
        Y[3:, :] = np.matmul(R, P[3:, :].reshape(N, 2, n)).reshape(2 * N, n)
    Z = Y.copy()
    Z[:, :2] = Y[:, :2] @ R.T
    if N:
        Z[:, 3:] = np.matmul(Y[:, 3:].reshape(n, N, 2), R.T).reshape(n, 2 * N)
    return Z


def frame_rows(x, T, absolute=False):
    """A (n x 3): the rows A_c of every item, from the OLD means; `absolute`: every factor by its absolute value."""
    x = np.asarray(x, dtype=float)
    n = len(x)
    R = rot(T[2])
    pts = np.vstack([x[:2], x[3:].reshape(-1, 2)])                # the pose's position, then the landmarks
    rp = np.abs(pts) @ np.abs(R).T if absolute else pts @ R.T      # R l  (|R| |l| for the bound)
    A = np.zeros((n, 3))
    rows = np.r_[0, 3 + 2 * np.arange((n - 3) // 2)]              # first row of every item
    A[rows, 0] = 1.0
    A[rows + 1, 1] = 1.0
    A[rows, 2] = rp[:, 1] if absolute else -rp[:, 1]
    A[rows + 1, 2] = rp[:, 0]
    A[2, 2] = 1.0
    return A


def transform_dense(x, P, T, cov=None):
    """(mean, covariance, covariance bound, mean bound) of the state moved through T."""
    x, P, T = np.asarray(x, dtype=float), np.asarray(P, dtype=float), np.asarray(T, dtype=float)
    R = rot(T[2])
    xn, mb = x.copy(), np.zeros_like(x)
    xn[:2] = T[:2] + R @ x[:2]
    xn[2] = x[2] + T[2]
    mb[:2] = np.abs(T[:2]) + np.abs(R) @ np.abs(x[:2])
    mb[2] = abs(x[2]) + abs(T[2])
    L = x[3:].reshape(-1, 2)
    xn[3:] = (T[:2] + L @ R.T).ravel()
    mb[3:] = (np.abs(T[:2]) + np.abs(L) @ np.abs(R).T).ravel()
    Pn = _congruence(P, R)
    bound = _congruence(np.abs(P), np.abs(R))
    if cov is not None:
        S = np.asarray(cov, dtype=float)
        A, Aa = frame_rows(x, T), frame_rows(x, T, absolute=True)
        Pn = Pn + A @ S @ A.T
        bound = bound + Aa @ np.abs(S) @ Aa.T
    return xn, Pn, bound, mb


ALIGN_FRAME = np.array([5.0, -3.0, 1.0])       # the filter's frame in the survey's
ALIGN_MARGIN = 1.5                             # tests: ate after align + anchor against ate(align=True) before


def align_case(N=20, steps=30, m=4, seed=41, noise=0.005):
    """The "align, then anchor" scenario of the CPU and the GPU tests: the dense oracle's state after `steps` steps over N
    landmarks, in the filter's own frame; a survey = the TRUE landmarks moved through ALIGN_FRAME plus `noise` (sigma, metres);
    two anchors with the survey's covariance."""
    from oracle import ekf_oracle as orc
    from tests import direct_model as dm
    _, x, P = dm.run_dense(N, steps, m, seed)
    _, lm, _, _ = orc.synthetic_world(N, seed)
    rng = np.random.default_rng(1000 + seed)
    survey = ALIGN_FRAME[:2] + lm @ rot(ALIGN_FRAME[2]).T + rng.normal(0.0, noise, lm.shape)
    return dict(x=x, P=P, survey=survey, anchors=(2, 11), R=np.eye(2) * noise ** 2)


def inverse(T):
    """The frame that undoes T."""
    R = rot(T[2])
    return np.r_[-(R.T @ np.asarray(T[:2], dtype=float)), -T[2]]


def compose(T2, T1):
    """The frame of applying T1, then T2."""
    return np.r_[np.asarray(T2[:2], dtype=float) + rot(T2[2]) @ np.asarray(T1[:2], dtype=float), T1[2] + T2[2]]
