"""The definition of a map join (EkfSlam.join, ekf_join_maps; k_join in csrc/ekf_join.hip), in NumPy, twice.

A base frame g = (t, phi) with covariance Sigma and cross terms G (3 x n_A, the covariance of g with A's state) maps every
item of the source B = [r_B; L_B] into the frame of the destination A = [r_A; L_A].  With R = rot(phi), J2 = [[0, -1], [1, 0]]:

    landmark  l' = t + R l                      A_l = [I2 | J2 R l]                B_l = R
    pose      p' = (t + R p_xy, phi + theta_B)  A_p = [[I2, J2 R p_xy], [0 0 1]]   B_p = diag(R, 1)

Sequential mode (transform None): g is A's pose, which is replaced by the composed pose; explicit mode: g = transform with
covariance `cov`, independent of both maps; A's pose stays and B's is dropped.

``join_dense`` is the textbook form: the Jacobian J of the whole map over [x_A; (T); x_B] and J P_in J^T with P_in block
diagonal.  ``join_closed`` is the block formula the kernel implements.  ``join_dense`` also returns the entrywise bounds
|J| |P_in| |J|^T and |t| + |R| |l| that the tests scale their tolerances by."""
import numpy as np

J2 = np.array([[0.0, -1.0], [1.0, 0.0]])


def rot(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.array([[c, -s], [s, c]])


def _items(xB, R, sequential):
    """Per mapped item of B: (its indices in x_B, A_c, B_c), the pose first in sequential mode."""
    out = []
    if sequential:
        A = np.zeros((3, 3))
        A[:2, :2] = np.eye(2)
        A[:2, 2] = J2 @ R @ xB[:2]
        A[2, 2] = 1.0
        B = np.eye(3)
        B[:2, :2] = R
        out.append((np.arange(3), A, B))
    for j in range((len(xB) - 3) // 2):
        idx = np.array([3 + 2 * j, 4 + 2 * j])
        A = np.hstack([np.eye(2), (J2 @ R @ xB[idx])[:, None]])
        out.append((idx, A, R))
    return out


def join_mean(xA, xB, transform=None):
    """(the joined mean, its entrywise bound |t| + |R| |l|; zero where an entry is only moved)."""
    seq = transform is None
    g = xA[:3] if seq else np.asarray(transform, dtype=float)
    R = rot(g[2])
    nA, NB = len(xA), (len(xB) - 3) // 2
    x, bound = np.zeros(nA + 2 * NB), np.zeros(nA + 2 * NB)
    x[:nA] = xA
    if seq:
        x[:2] = g[:2] + R @ xB[:2]
        x[2] = g[2] + xB[2]
        bound[:2] = np.abs(g[:2]) + np.abs(R) @ np.abs(xB[:2])
        bound[2] = abs(g[2]) + abs(xB[2])
    for j in range(NB):
        l = xB[3 + 2 * j:5 + 2 * j]
        x[nA + 2 * j:nA + 2 * j + 2] = g[:2] + R @ l
        bound[nA + 2 * j:nA + 2 * j + 2] = np.abs(g[:2]) + np.abs(R) @ np.abs(l)
    return x, bound


def join_dense(xA, PA, xB, PB, transform=None, cov=None, with_bound=True):
    """(mean, covariance, covariance bound, mean bound) by the dense product J P_in J^T (``with_bound`` False: no second
    product, None in its place)."""
    seq = transform is None
    nA, nB = len(xA), len(xB)
    NB = (nB - 3) // 2
    g = xA[:3] if seq else np.asarray(transform, dtype=float)
    R = rot(g[2])
    nT = 0 if seq else 3
    n_in, n_out = nA + nT + nB, nA + 2 * NB
    P_in = np.zeros((n_in, n_in))
    P_in[:nA, :nA] = PA
    if not seq:
        P_in[nA:nA + 3, nA:nA + 3] = np.zeros((3, 3)) if cov is None else cov
    P_in[nA + nT:, nA + nT:] = PB
    J = np.zeros((n_out, n_in))
    J[:nA, :nA] = np.eye(nA)
    gcols = np.arange(3) if seq else nA + np.arange(3)
    row = nA
    for idx, A, B in _items(xB, R, seq):
        if len(idx) == 3:                              # the pose replaces A's
            rows = np.arange(3)
            J[np.ix_(rows, np.arange(3))] = 0.0
        else:
            rows = np.arange(row, row + 2)
            row += 2
        J[np.ix_(rows, gcols)] = A
        J[np.ix_(rows, nA + nT + idx)] = B
    P = J @ P_in @ J.T
    bound = np.abs(J) @ np.abs(P_in) @ np.abs(J).T if with_bound else None
    x, mbound = join_mean(xA, xB, transform)
    return x, P, bound, mbound


def join_closed(xA, PA, xB, PB, transform=None, cov=None, bound=False):
    """(mean, covariance) by the block formulas: P'[c1, c2] = A_c1 Sigma A_c2^T + B_c1 P_B[c1, c2] B_c2^T and
    P'[a, c] = G[:, a]^T A_c^T for a kept index a; P'[L_A, L_A] unchanged.  ``bound``: every factor by its absolute value
    -- the covariance returned is then join_dense's bound |J| |P_in| |J|^T, without the dense product (large states)."""
    seq = transform is None
    if bound:
        PA, PB = np.abs(PA), np.abs(PB)
        cov = None if cov is None else np.abs(cov)
    nA = len(xA)
    NB = (len(xB) - 3) // 2
    if seq:
        g, Sigma, G = xA[:3], PA[:3, :3], PA[:3, :]
    else:
        g = np.asarray(transform, dtype=float)
        Sigma = np.zeros((3, 3)) if cov is None else np.asarray(cov, dtype=float)
        G = np.zeros((3, nA))
    R = rot(g[2])
    n = nA + 2 * NB
    P = np.zeros((n, n))
    P[:nA, :nA] = PA
    items, row = [], nA
    for idx, A, B in _items(xB, R, seq):
        if len(idx) == 3:
            rows = np.arange(3)
        else:
            rows = np.arange(row, row + 2)
            row += 2
        items.append((rows, idx, np.abs(A), np.abs(B)) if bound else (rows, idx, A, B))
    kept = np.arange(3 if seq else 0, nA)
    for rows, idx, A, B in items:
        P[np.ix_(kept, rows)] = G[:, kept].T @ A.T
        P[np.ix_(rows, kept)] = A @ G[:, kept]
    for r1, i1, A1, B1 in items:
        for r2, i2, A2, B2 in items:
            P[np.ix_(r1, r2)] = A1 @ Sigma @ A2.T + B1 @ PB[np.ix_(i1, i2)] @ B2.T
    return join_mean(xA, xB, transform)[0], P


def random_state(rng, N, never_observed=None, scale=0.3):
    """A dense positive definite state of N landmarks; `never_observed`: that landmark has variance 1e4 and no correlations."""
    n = 3 + 2 * N
    A = rng.normal(size=(n, n)) * scale
    P = A @ A.T + np.diag(rng.uniform(0.01, 0.1, n))
    x = rng.uniform(-3.0, 3.0, n)
    x[2] = rng.uniform(-np.pi, np.pi)
    if never_observed is not None and N > 0:
        i = 3 + 2 * never_observed
        P[i:i + 2, :] = 0.0
        P[:, i:i + 2] = 0.0
        P[i, i] = P[i + 1, i + 1] = 1e4
    return x, P


def random_frame(rng):
    """(transform, cov): a frame with a positive definite covariance."""
    A = rng.normal(size=(3, 3)) * 0.1
    return np.r_[rng.uniform(-2.0, 2.0, 2), rng.uniform(-np.pi, np.pi)], A @ A.T + np.diag([1e-3, 1e-3, 1e-4])
