"""GPU: the Cholesky factor of the whole covariance on the device (ekf_factor, ekf_factor_solve, ekf_factor_multiply,
ekf_download_factor, ekf_factor_release; EkfSlam.factor / CovFactor) and evaluation.map_nees on top of it.

States are uploaded with set_state from seeded SPD matrices "diagonal + low rank" (tests/factor_model.py: spd, kappa_2 about
3 n / 8, below 1e4) unless a case says otherwise.  Tolerances (eps = 2^-53, gamma_k = k eps / (1 - k eps)):
  structure    U strictly upper triangular with a positive diagonal
  residual     |U^T U - P|_F <= gamma_{n+1} | |U^T| |U| |_F      Higham's backward bound for Cholesky: any summation order
  logdet       |logdet - 2 sum ln diag chol_numpy(P)| <= 2 n gamma_{n+1} kappa_2(P)
               (a backward error dP moves ln det by at most n |P^-1| |dP|, once for each side)
  solve        quad and white relative to NumPy's: <= 10 n eps kappa_2(P)  (first-order forward bound of a triangular solve,
               device and reference, plus constants)
  round trip   |multiply(whiten(e)) - e| / |e| <= (10 n eps kappa + gamma_n sqrt(n)) sqrt(kappa): the solve's relative
               error c in w is amplified by |U| |w| <= sqrt(kappa) |e| (|w| <= |U^-1| |e|), the product's own error is
               gamma_n | |U^T| |w| | <= gamma_n sqrt(n) |U| |w|
Every check prints its measured ratio to the bound.  Claims of bit-identity are exact (np.array_equal)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import factor_model as fm
from tests.conftest import path_ran
from tests.factor_model import EPS, check_factor, gamma
from tests.gpu_support import sd  # noqa: F401

pytestmark = pytest.mark.gpu

EKF_ERR_ARG, EKF_ERR_STATE = -1, -3
_dp = C.POINTER(C.c_double)


def upload(f, b, P, seed=0):
    mean = np.random.default_rng(1000 + seed).standard_normal(P.shape[0])
    f.set_state(mean, P, b)
    return mean


def test_after_a_stream_on_both_paths(sd, both_paths):
    """N = 20 (n = 43) x 3 after a synthetic stream that leaves ranks pending on the general kernels: U, logdet and info
    against NumPy on covariance(b).  Small states are one diagonal-block launch; the small-state path's triangle in HBM is
    current after the flush."""
    N, B, steps = 20, 3, 3
    streams = [orc.synthetic_stream(N, steps, 8, 70 + t) for t in range(B)]
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_option("fused_cadence", 0)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        for k in range(steps):
            f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                   np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
                   np.stack([s[6][k] for s in streams]))
        assert path_ran(f, both_paths)
        fac = f.factor()
        assert (fac.info == 0).all() and fac.n.tolist() == [43] * B
        for b in range(B):
            check_factor(f"{both_paths} b = {b}", fac.upper(b), fac.logdet[b], f.covariance(b))
            assert np.array_equal(fac.means[b], f.mean(b))
        assert path_ran(f, both_paths)


@pytest.mark.parametrize("N", [30, 31, 94, 95])
def test_block_edges(sd, N):
    """n = 63, 65, 191, 193 on the general kernels: one below and one above a whole number of blocks."""
    n = 3 + 2 * N
    P, _ = fm.spd(n, n)
    with sd.EkfSlam(n) as f:
        f.set_option("small_state", 0)
        upload(f, 0, P)
        fac = f.factor(0)
        assert fac.info[0] == 0
        check_factor(f"n = {n}", fac.upper(0), fac.logdet[0], f.covariance(0))
        assert np.array_equal(f.covariance(0), P)


def test_fresh_handle_n3(sd):
    with sd.EkfSlam(3 + 2 * 40) as f:
        fac = f.factor()
        assert fac.n.tolist() == [3] and fac.info[0] == 0
        check_factor("n = 3", fac.upper(0), fac.logdet[0], f.covariance(0))


def test_ragged_bank_and_ranges_bit_identical(sd):
    """One bank with n = 3, 43 and 193 (n_max = 203): the whole bank, then the sub-range b0 = 1, count = 2 -- every
    trajectory's U is bit-identical in both, and to the same state factored alone in another handle."""
    P1, _ = fm.spd(43, 1)
    P2, _ = fm.spd(193, 2)
    with sd.EkfSlam(203, batch=3) as f:
        upload(f, 1, P1)
        upload(f, 2, P2)
        fac = f.factor()
        assert fac.n.tolist() == [3, 43, 193] and (fac.info == 0).all()
        whole = [fac.upper(b) for b in range(3)]
        logdet = fac.logdet.copy()
        for b, P in ((1, P1), (2, P2)):
            check_factor(f"bank b = {b}", whole[b], logdet[b], P)
        lib = sd.load_library()
        ld, info = np.empty(2), np.empty(2, dtype=np.int32)
        assert lib.ekf_factor(f._h, 1, 2, ld.ctypes.data_as(_dp), info.ctypes.data_as(C.POINTER(C.c_int))) == 0
        assert np.array_equal(ld, logdet[1:]) and (info == 0).all()
        for b in (1, 2):
            U = np.empty((fac.n[b], fac.n[b]))
            assert lib.ekf_download_factor(f._h, b, U.ctypes.data_as(_dp), int(fac.n[b])) == 0
            assert np.array_equal(U, whole[b])
        U = np.empty((3, 3))
        assert lib.ekf_download_factor(f._h, 0, U.ctypes.data_as(_dp), 3) == EKF_ERR_STATE   # outside the factored range now
    for b, P in ((0, None), (1, P1), (2, P2)):
        with sd.EkfSlam(3 if P is None else P.shape[0]) as g:
            g.set_option("small_state", 0)
            if P is not None:
                upload(g, 0, P)
            alone = g.factor(0)
            assert np.array_equal(alone.upper(0), whole[b]) and alone.logdet[0] == logdet[b]


def test_column_panel_boundary(sd):
    """n_max = 4203 (ld > 4096: the covariance lies in column panels), n = 4103: 65 block steps and a panel crossing."""
    n = 4103
    P, kappa = fm.spd(n, 4, const_diag=True)                # (constant diagonal: kappa_2 = (d + sigma_1(V)^2) / d exactly)
    with sd.EkfSlam(4203) as f:
        upload(f, 0, P)
        fac = f.factor(0)
        assert fac.info[0] == 0 and fac.n[0] == n
        check_factor("n = 4103", fac.upper(0), fac.logdet[0], P, kappa)


def test_not_positive_definite(sd):
    """A negative pivot inside the first block (index 50), one that turns negative only after a trailing down-date (index
    100) and a NaN entry: info equals the model's, every output of that trajectory is NaN, and the other trajectories are
    bit-identical to a bank without the bad ones."""
    n = 193
    good = [fm.spd(n, 20)[0], fm.spd(n, 21)[0]]
    base = fm.spd(n, 22)[0]
    bad50, bad100, badnan = fm.not_pd_at(base, 50), fm.not_pd_at(base, 100), base.copy()
    badnan[10, 150] = np.nan
    assert bad100[100, 100] > 0
    bank = [good[0], bad50, good[1], bad100, badnan]
    want = [fm.blocked_cholesky(P)[2] for P in bank]
    assert want == [0, 51, 0, 101, 151]
    with sd.EkfSlam(n, batch=5) as f, sd.EkfSlam(n, batch=2) as g:
        for b, P in enumerate(bank):
            upload(f, b, P, b)
        upload(g, 0, good[0], 0)
        upload(g, 1, good[1], 2)
        fac = f.factor()
        assert fac.info.tolist() == want
        assert np.isnan(fac.logdet[[1, 3, 4]]).all() and np.isfinite(fac.logdet[[0, 2]]).all()
        e = np.random.default_rng(3).standard_normal((5, 2, n))
        white, quad, prod = fac.whiten(e), fac.mahalanobis(e), fac.multiply(e)
        for b in (1, 3, 4):
            assert np.isnan(white[b]).all() and np.isnan(quad[b]).all() and np.isnan(prod[b]).all()
            with pytest.raises(sd.EkfError, match="not positive definite"):
                fac.upper(b)
            assert f.flags(b) == 0                           # a query: no sticky flag
        for b in (0, 2):
            assert np.isfinite(white[b]).all() and np.isfinite(quad[b]).all() and np.isfinite(prod[b]).all()
        kept = [fac.upper(0), fac.upper(2)]
        clean = g.factor()
        assert (clean.info == 0).all()
        for i, b in enumerate((0, 2)):
            assert np.array_equal(clean.upper(i), kept[i]) and clean.logdet[i] == fac.logdet[b]
            assert np.array_equal(clean.whiten(e[[0, 2]])[i], white[b]) and np.array_equal(clean.multiply(e[[0, 2]])[i], prod[b])


def test_factor_leaves_the_filter_where_a_flush_would(sd):
    """Two handles run the same stream; at the same step one calls factor(), the other flush(): the final state() is
    bit-identical, cadence_counters() and profile_passes() are equal."""
    N, B, steps = 150, 2, 6
    streams = [orc.synthetic_stream(N, steps, 8, 90 + t) for t in range(B)]

    def run(query):
        with sd.EkfSlam(3 + 2 * N, batch=B) as f:
            f.profile_enable(True)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            for k in range(steps):
                f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                       np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
                       np.stack([s[6][k] for s in streams]))
                if k == 2:
                    query(f)
            return [f.state(b) for b in range(B)], f.cadence_counters(), f.profile_passes()

    def factored(f):
        assert (f.factor().info == 0).all()

    a, b = run(factored), run(lambda f: f.flush())
    assert a[1] == b[1] and a[2] == b[2] and a[2] >= 1
    for t in range(B):
        assert np.array_equal(a[0][t][0], b[0][t][0]) and np.array_equal(a[0][t][1], b[0][t][1])


def test_factor_is_a_snapshot(sd):
    """Stepping the filter after factor() leaves upper(b) bit for bit; a second factor() differs and invalidates the first."""
    N = 150
    s = orc.synthetic_stream(N, 4, 8, 95)
    with sd.EkfSlam(3 + 2 * N) as f:
        f.set_state_diag(s[0], s[1])
        for k in range(2):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        fac = f.factor(0)
        U0, w0 = fac.upper(0), fac.whiten(np.ones(fac.n[0]))
        for k in range(2, 4):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        f.flush()
        assert np.array_equal(fac.upper(0), U0) and np.array_equal(fac.whiten(np.ones(fac.n[0])), w0)
        newer = f.factor(0)
        assert not np.array_equal(newer.upper(0), U0)
        with pytest.raises(sd.EkfError, match="replaced"):
            fac.upper(0)
        f.release_factor()
        with pytest.raises(sd.EkfError, match="replaced"):
            newer.mahalanobis(np.ones(newer.n[0]))


@pytest.mark.parametrize("nrhs", [1, 16])
def test_solve_and_multiply(sd, nrhs):
    """nrhs = 1 and 16 with stride > n (the bank's 43-state trajectory under the stride of 193, and the C ABI called with
    stride = n + 7): quad and white against np.linalg.solve, multiply(whiten(e)) = e, multiply(I)^T multiply(I) = P."""
    sizes = (43, 193)
    mats = [fm.spd(n, 30 + n) for n in sizes]
    rng = np.random.default_rng(nrhs)
    with sd.EkfSlam(193, batch=2) as f:
        for b, (P, _) in enumerate(mats):
            upload(f, b, P, b)
        fac = f.factor()
        e = rng.standard_normal((2, nrhs, 193))
        white, quad = fac.whiten(e), fac.mahalanobis(e)
        back = fac.multiply(np.nan_to_num(white))
        for b, (P, _) in enumerate(mats):
            n, kappa = sizes[b], np.linalg.cond(P)
            L = np.linalg.cholesky(P)
            wref = np.linalg.solve(L, e[b, :, :n].T).T
            qref = np.einsum("ki,ik->k", e[b, :, :n], np.linalg.solve(P, e[b, :, :n].T))
            bound = 10 * n * EPS * kappa
            rw = np.linalg.norm(white[b, :, :n] - wref, axis=1) / np.linalg.norm(wref, axis=1) / bound
            rq = np.abs(quad[b] - qref) / qref / bound
            rt = (np.linalg.norm(back[b, :, :n] - e[b, :, :n], axis=1) / np.linalg.norm(e[b, :, :n], axis=1)
                  / ((bound + gamma(n) * np.sqrt(n)) * np.sqrt(kappa)))
            print(f"nrhs = {nrhs} n = {n} kappa = {kappa:.3g}: white / bound {rw.max():.3g} quad / bound {rq.max():.3g} "
                  f"round trip / bound {rt.max():.3g}")
            assert rw.max() <= 1 and rq.max() <= 1 and rt.max() <= 1
            assert np.isnan(white[b, :, n:]).all() and np.isnan(back[b, :, n:]).all()
        # the C ABI with a stride of its own, one trajectory of the range, white or quad alone
        lib, n = sd.load_library(), 43
        stride = n + 7
        rhs = np.ascontiguousarray(np.pad(e[0, :, :n], ((0, 0), (0, 7)), constant_values=np.nan))   # (beyond n: never read)
        w2, q2 = np.zeros((nrhs, stride)), np.zeros(nrhs)
        assert lib.ekf_factor_solve(f._h, 0, 1, rhs.ctypes.data_as(_dp), nrhs, stride, w2.ctypes.data_as(_dp), None) == 0
        assert lib.ekf_factor_solve(f._h, 0, 1, rhs.ctypes.data_as(_dp), nrhs, stride, None, q2.ctypes.data_as(_dp)) == 0
        assert np.array_equal(w2[:, :n], white[0, :, :n]) and np.isnan(w2[:, n:]).all() and np.array_equal(q2, quad[0])
        o2 = np.zeros((nrhs, stride))
        assert lib.ekf_factor_multiply(f._h, 0, 1, np.nan_to_num(w2).ctypes.data_as(_dp), nrhs, stride, o2.ctypes.data_as(_dp)) == 0
        assert np.array_equal(o2[:, :n], back[0, :, :n]) and np.isnan(o2[:, n:]).all()
        if nrhs == 16:
            for b, (P, _) in enumerate(mats):
                n = sizes[b]
                eye = np.zeros((2, n, 193))
                eye[b, :, :n] = np.eye(n)
                M = fac.multiply(eye)[b, :, :n]              # row i = U^T e_i = row i of U
                assert np.array_equal(M, fac.upper(b))
                res = np.linalg.norm(M.T @ M - P) / (gamma(n + 1) * np.linalg.norm(np.abs(M.T) @ np.abs(M)))
                print(f"multiply(I)^T multiply(I) - P, n = {n}: residual / bound = {res:.3g}")
                assert res <= 1


def test_errors(sd):
    lib = sd.load_library()
    P, _ = fm.spd(43, 7)
    x = np.ones((2, 16, 64))
    px = x.ctypes.data_as(_dp)
    out, quad = np.empty((2, 16, 64)), np.empty((2, 16))
    po, pq = out.ctypes.data_as(_dp), quad.ctypes.data_as(_dp)
    with sd.EkfSlam(43, batch=3) as f:
        for b in range(3):
            upload(f, b, P, b)
        assert lib.ekf_factor_solve(f._h, 0, 1, px, 1, 64, po, pq) == EKF_ERR_STATE        # before any factor
        assert lib.ekf_factor_multiply(f._h, 0, 1, px, 1, 64, po) == EKF_ERR_STATE
        assert lib.ekf_download_factor(f._h, 0, po, 43) == EKF_ERR_STATE
        ld, info = np.empty(3), np.empty(3, dtype=np.int32)
        pl, pi = ld.ctypes.data_as(_dp), info.ctypes.data_as(C.POINTER(C.c_int))
        for b0, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
            assert lib.ekf_factor(f._h, b0, count, pl, pi) == EKF_ERR_ARG
        assert lib.ekf_factor(f._h, 0, 2, None, None) == 0                                  # either output may be NULL
        assert lib.ekf_factor_solve(f._h, 0, 2, px, 16, 64, po, pq) == 0
        for nrhs, stride in ((0, 64), (17, 64), (1, 42), (1, 0), (1, -5)):
            assert lib.ekf_factor_solve(f._h, 0, 2, px, nrhs, stride, po, pq) == EKF_ERR_ARG
            assert lib.ekf_factor_multiply(f._h, 0, 2, px, nrhs, stride, po) == EKF_ERR_ARG
        for b0, count in ((-1, 1), (0, 0), (0, 4), (3, 1)):                                  # outside the bank
            assert lib.ekf_factor_solve(f._h, b0, count, px, 1, 64, po, pq) == EKF_ERR_ARG
        assert lib.ekf_factor_solve(f._h, 1, 2, px, 1, 64, po, pq) == EKF_ERR_STATE         # inside the bank, outside the factor
        assert lib.ekf_factor_solve(f._h, 0, 2, None, 1, 64, po, pq) == EKF_ERR_ARG
        assert lib.ekf_factor_solve(f._h, 0, 2, px, 1, 64, None, None) == EKF_ERR_ARG
        assert lib.ekf_factor_multiply(f._h, 0, 2, px, 1, 64, None) == EKF_ERR_ARG
        bad = x.copy()
        bad.reshape(-1)[1 * 1 * 64 + 42] = np.inf              # (count x nrhs x stride with nrhs = 1: entry 42 of trajectory 1)
        assert lib.ekf_factor_solve(f._h, 0, 2, bad.ctypes.data_as(_dp), 1, 64, po, pq) == EKF_ERR_ARG
        assert b"non-finite" in lib.ekf_last_error(f._h)
        for n in (41, 45, 0):
            assert lib.ekf_download_factor(f._h, 0, po, n) == EKF_ERR_ARG
        assert lib.ekf_download_factor(f._h, 0, None, 43) == EKF_ERR_ARG
        assert lib.ekf_download_factor(f._h, 3, po, 43) == EKF_ERR_ARG
        assert lib.ekf_download_factor(f._h, 2, po, 43) == EKF_ERR_STATE
        # ... with the handle usable and the factor still held
        q0 = quad.copy()
        assert lib.ekf_factor_solve(f._h, 0, 2, px, 16, 64, po, pq) == 0 and np.array_equal(quad, q0)
        assert lib.ekf_factor_release(f._h) == 0 and lib.ekf_factor_release(f._h) == 0
        assert lib.ekf_factor_solve(f._h, 0, 2, px, 16, 64, po, pq) == EKF_ERR_STATE        # after the release
        assert (f.factor().info == 0).all()


def test_map_nees_equals_the_oracle_banks(sd):
    """evaluation.map_nees on a bank of 4 at N = 20 against e^T P^-1 e from the oracle bank's dense P."""
    from slam_duckietown_amd import evaluation as ev
    N, B, steps = 20, 4, 5
    cfg = orc.EkfConfig()
    rng = np.random.default_rng(11)
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        streams = [orc.synthetic_stream(N, steps, 8, 60 + t) for t in range(B)]
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        for k in range(steps):
            f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                   np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
                   np.stack([s[6][k] for s in streams]))
        poses, lms = rng.standard_normal((B, 3)), rng.standard_normal((B, N, 2)) * 3
        r = ev.map_nees(f, poses, lms)
        assert r.dof.tolist() == [43] * B and (r.info == 0).all() and r.bounds == ev.chi2_bounds(43, B, 0.95)
        for b, s in enumerate(streams):
            om, oP = s[0].copy(), np.diag(s[1])
            for k in range(steps):
                om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
            e = om - np.concatenate([poses[b], lms[b].reshape(-1)])
            e[2] = ev.wrap_angle(e[2])
            want = e @ np.linalg.solve(oP, e)
            # the filter's state equals the oracle's to 1e-9 (the parity tests' bound); through the solve with kappa_2(P)
            bound = 1e-9 * np.linalg.cond(oP)
            print(f"map_nees b = {b}: {r.nees[b]:.6g} against {want:.6g}, relative difference / bound = "
                  f"{abs(r.nees[b] - want) / want / bound:.3g}")
            assert abs(r.nees[b] - want) <= bound * want
        assert r.anees == pytest.approx(r.nees.mean())
