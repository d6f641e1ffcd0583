"""NumPy restatement of the device's blocked Cholesky factorisation (csrc/ekf_factor.hip): right-looking, block 64, the
ragged last block padded with an identity diagonal, `info` as LAPACK dpotrf (0, or the 1-based index of the first pivot
that is <= 0 or not finite).  Only the upper triangle of P is read, as on the device.  Also a stand-in filter whose
`factor()` is backed by this model, for the host-side code on top of it (CovFactor's generation check, evaluation.map_nees,
map_entropy) where there is no GPU, and the seeded test matrices both test files use."""
import numpy as np

FB = 64
EPS = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k eps / (1 - k eps), the unit of both test files' bounds."""
    return k * EPS / (1.0 - k * EPS)


def blocked_cholesky(P):
    """(U, logdet, info) of P = U^T U as the device forms them; U and logdet are NaN where info != 0."""
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[0]
    nblk = (n + FB - 1) // FB
    lw = nblk * FB
    A = np.zeros((lw, lw))
    A[:n, :n] = np.triu(P)
    A[np.arange(n, lw), np.arange(n, lw)] = 1.0
    logdet = 0.0
    for k in range(nblk):
        lo, hi = k * FB, (k + 1) * FB
        D = A[lo:hi, lo:hi]
        for j in range(FB):                                 # the diagonal block, unblocked
            piv = D[j, j]
            if not (piv > 0.0) or not np.isfinite(piv):
                return np.full((n, n), np.nan), float("nan"), lo + j + 1
            d = np.sqrt(piv)
            if lo + j < n:
                logdet += 2.0 * np.log(d)
            D[j, j] = d
            D[j, j + 1:] /= d
            D[j, :j] = 0.0
            r = np.arange(j + 1, FB)
            D[j + 1:, j + 1:] -= np.triu(np.outer(D[j, r], D[j, r]))
        A[lo:hi, lo:hi] = np.triu(D)
        if hi == lw:
            break
        L = D.T                                             # the row panel, by forward substitution with U_kk^T
        X = A[lo:hi, hi:]
        for r in range(FB):
            X[r] = (X[r] - L[r, :r] @ X[:r]) / L[r, r]
        with np.errstate(invalid="ignore", over="ignore"):
            A[hi:, hi:] -= np.triu(X.T @ X)                 # the trailing down-date, tiles i <= j
    return A[:n, :n].copy(), logdet, 0


def check_factor(name, U, logdet, P, kappa=None):
    """Structure, residual and log-determinant of one trajectory's factor against P; prints the ratios to the bounds."""
    n = P.shape[0]
    assert U.shape == (n, n) and np.array_equal(U, np.triu(U)) and (np.diag(U) > 0).all()
    kappa = np.linalg.cond(P) if kappa is None else kappa
    res = np.linalg.norm(U.T @ U - P) / (gamma(n + 1) * np.linalg.norm(np.abs(U.T) @ np.abs(U)))
    ref = 2.0 * np.log(np.diag(np.linalg.cholesky(P))).sum()
    dl = abs(logdet - ref) / (2 * n * gamma(n + 1) * kappa)
    print(f"{name}: n = {n} kappa = {kappa:.3g} residual / bound = {res:.3g} logdet error / bound = {dl:.3g}")
    assert res <= 1.0 and dl <= 1.0


def spd(n, seed, rank=8, const_diag=False):
    """A seeded SPD matrix "diagonal + low rank", D + V V^T with D in [1, 2] and rows of V of squared length about 3 (so that
    eliminating the rows above an entry takes most of its diagonal away): kappa_2 is about 3 n / 8, 100 at n = 193 and 1700 at
    n = 4103, below 1e4.  Returns (P exactly symmetric, an upper bound of kappa_2 that is exact with const_diag)."""
    rng = np.random.default_rng(seed)
    d = np.full(n, 1.5) if const_diag else rng.uniform(1.0, 2.0, n)
    V = rng.standard_normal((n, rank)) * np.sqrt(3.0 / rank)
    P = V @ V.T
    P = np.triu(P) + np.triu(P, 1).T
    P[np.arange(n), np.arange(n)] += d
    s1 = np.linalg.svd(V, compute_uv=False)[0]
    return P, (d.max() + s1 * s1) / d.min()


def not_pd_at(P, index):
    """P with its diagonal entry `index` lowered so that exactly that pivot of the factorisation turns negative (a quarter of its
    value), every earlier one untouched."""
    U = np.linalg.cholesky(P).T
    out = P.copy()
    out[index, index] -= 1.25 * U[index, index] ** 2
    return out


class ModelFactorFilter:
    """What CovFactor and evaluation.map_nees use of an EkfSlam, backed by blocked_cholesky: `_lib` is the object itself."""

    def __init__(self, means, covs):
        self.batch = len(means)
        self._means = [np.asarray(m, dtype=float) for m in means]
        self._covs = [np.asarray(P, dtype=float) for P in covs]
        self._lib, self._h = self, None
        self._factor_generation = 0
        self._U = None

    def _check(self, rc):
        assert rc == 0

    def size(self, b=0):
        return len(self._means[b])

    def mean(self, b=0):
        return self._means[b].copy()

    def factor(self, b=None):
        from slam_duckietown_amd.ekf_bindings import CovFactor
        b0, count = (0, self.batch) if b is None else (int(b), 1)
        res = [blocked_cholesky(self._covs[t]) for t in range(b0, b0 + count)]
        self._U = {b0 + i: r[0] for i, r in enumerate(res)}
        self._info = {b0 + i: r[2] for i, r in enumerate(res)}
        self._factor_generation += 1
        n = np.array([self.size(t) for t in range(b0, b0 + count)], dtype=np.int32)
        return CovFactor(self, self._factor_generation, b0, count, b is not None, np.array([r[1] for r in res]),
                         np.array([r[2] for r in res], dtype=np.int32), n, [self.mean(t) for t in range(b0, b0 + count)])

    def release_factor(self):
        self._factor_generation += 1
        self._U = None

    # the three entry points CovFactor calls, on ctypes pointers
    @staticmethod
    def _arr(ptr, shape):
        return np.ctypeslib.as_array(ptr, shape=shape)

    def ekf_factor_solve(self, h, b0, count, rhs, nrhs, stride, white, quad):
        r = self._arr(rhs, (count, nrhs, stride))
        for bi in range(count):
            U, n = self._U[b0 + bi], self.size(b0 + bi)
            w = np.full((nrhs, stride), np.nan)
            if self._info[b0 + bi] == 0:
                w[:, :n] = np.linalg.solve(U.T, r[bi, :, :n].T).T
            if white:
                self._arr(white, (count, nrhs, stride))[bi] = w
            self._arr(quad, (count, nrhs))[bi] = (w[:, :n] ** 2).sum(axis=1)
        return 0

    def ekf_factor_multiply(self, h, b0, count, z, nrhs, stride, out):
        x = self._arr(z, (count, nrhs, stride))
        for bi in range(count):
            U, n = self._U[b0 + bi], self.size(b0 + bi)
            o = np.full((nrhs, stride), np.nan)
            if self._info[b0 + bi] == 0:
                o[:, :n] = x[bi, :, :n] @ U
            self._arr(out, (count, nrhs, stride))[bi] = o
        return 0

    def ekf_download_factor(self, h, b, U, n):
        self._arr(U, (n, n))[:] = self._U[b]
        return 0
