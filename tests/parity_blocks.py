"""Block-wise parity of a filter state against a reference state (the oracle's, or another path's).

From a block-diagonal start (`set_state_diag`: pose variance 0.1, every landmark 1e4) the whole-matrix relative Frobenius
distance is dominated by the landmarks nobody has observed yet: at N = 2000 after 12 steps |P|_F is 6.2e5 and the pose
block 0.34, so a pose block 0.1 % off moves the whole-matrix metric by 5e-10 and passes a 1e-9 check.  The mean has the same
problem (|mu| ~ 39, the pose ~ 0.2).  `assert_filter_close` compares the pieces a filter is made of, each on its own scale:

covariance, on the ACTIVE part (pose + observed landmarks):
  pose block (3 x 3), pose-landmark cross rows (3 x observed), observed landmark-landmark block: relative Frobenius error;
  correlation-scaled maximum  max |dP_ij| / sqrt(oP_ii oP_jj)  (independent of how large the entries are);
mean:
  pose: relative error;  observed landmarks: max |dmu_i| / sqrt(oP_ii);
never-observed landmarks (block-diagonal start: `mean0` / `diag0` given):
  mean and variance bit-equal to the start, every off-diagonal entry of their rows and columns exactly 0.

`assert_update_close` judges ONE direct or linear update applied to a known state the same way: the landmarks fall into three
classes by the state the call found -- active before the call (the pieces above), never observed and first touched by this call
(own block within 32 eps landmark_init_var, mean within 1e-9, cross terms exact zeros for a direct fix and entrywise for a dense
H), never observed and not named (mean, variance and whole rows bit for bit, exact zeros) -- and P must be exactly symmetric.

`assert_state_close` judges a WHOLE state after any sequence of calls against a dense model fed the same calls: the landmarks
are classed by the model's state, not by history -- loose (both variances still at or above half of landmark_init_var: own block
within 32 eps landmark_init_var, mean within 1e-9, cross terms exactly zero where the model's are, entrywise elsewhere) and
informed (with the pose: the pieces above) -- plus exact symmetry, size, tag index and flags.

Every assertion message names the piece and the measured value.  A plain module (not a conftest): tests import it.
"""
import numpy as np

REL_TOL = 1e-6          # the north-star bar (BASELINE.json): never relaxed, whatever `tol` says
# The two per-entry maxima (corr_max, mean_landmarks) between two GPU paths from a block-diagonal start: a landmark's first
# update cancels its 1e4 prior variance down to ~0.5, so a last-bit difference in the order of summation leaves
# ~eps * 1e4 = 2e-12 on an entry of that size (the oracle run twice on the CPU, one run symmetrised after every step: corr_max
# 8.7e-12, mean_landmarks 1.4e-12 after 100 steps at N = 2000, whole matrix 9e-17; measured between the GPU paths: up to
# 2.3e-11 and 1.8e-11).  The paths' relative Frobenius pieces stay at the callers' 1e-11; the largest single entry is held
# to the 1e-10 the cadence header guarantees between paths.
PATH_CORR_TOL = 1e-10

PIECES = ("pose", "cross", "landmarks", "corr_max", "mean_pose", "mean_landmarks")


def observed_landmarks(idx, m=None):
    """Sorted landmark indices a stream observes: idx [steps, (batch,) stride] with, for variable streams, m [steps, (batch)]
    the number of valid entries per step (entries beyond it are padding and not observed)."""
    idx = np.asarray(idx)
    if m is None:
        return np.unique(idx)
    m = np.asarray(m)
    valid = np.arange(idx.shape[-1]) < m[..., None]
    return np.unique(idx[valid])


def landmark_rows(observed):
    """State indices (x and y rows) of the landmarks `observed`."""
    observed = np.asarray(observed, dtype=np.int64)
    return np.stack([3 + 2 * observed, 4 + 2 * observed], axis=1).ravel()


def _rel(a, b):
    den = np.linalg.norm(b)
    num = np.linalg.norm(np.asarray(a) - np.asarray(b))
    return float(num / den) if den > 0 else float(num)


def active_errors(mu_a, P_a, om_a, oP_a):
    """The block-wise errors of an active part: index 0..2 the pose, the rest observed landmarks' state rows (P_a, oP_a
    square over the same indices).  -> {piece: measured value}."""
    P_a, oP_a = np.asarray(P_a, dtype=float), np.asarray(oP_a, dtype=float)
    mu_a, om_a = np.asarray(mu_a, dtype=float), np.asarray(om_a, dtype=float)
    d = np.diag(oP_a)
    if not (d > 0).all():
        raise AssertionError("reference covariance has a non-positive variance on the active part")
    scale = np.sqrt(np.outer(d, d))
    err = {"pose": _rel(P_a[:3, :3], oP_a[:3, :3]),
           "corr_max": float(np.max(np.abs(P_a - oP_a) / scale)),
           "mean_pose": _rel(mu_a[:3], om_a[:3])}
    if len(mu_a) > 3:
        err["cross"] = _rel(P_a[:3, 3:], oP_a[:3, 3:])
        err["landmarks"] = _rel(P_a[3:, 3:], oP_a[3:, 3:])
        err["mean_landmarks"] = float(np.max(np.abs(mu_a[3:] - om_a[3:]) / np.sqrt(d[3:])))
    return err


def check_errors(err, tol, what="", corr_tol=None):
    """Every piece below the 1e-6 bar and below `tol` (the per-entry maxima corr_max and mean_landmarks: `corr_tol` where
    given); the message lists every piece that is not."""
    lim = {p: (corr_tol if p in ("corr_max", "mean_landmarks") and corr_tol is not None else tol) for p in PIECES}
    bad = [f"{what}{p}: {err[p]:.3e} exceeds " + ("the 1e-6 bar" if err[p] >= REL_TOL else f"the expected {lim[p]:g}")
           for p in PIECES if p in err and not (err[p] < REL_TOL and err[p] < lim[p])]
    assert not bad, "; ".join(bad)


def assert_symmetric(P_a, tol, what=""):
    """max |P_ij - P_ji| / sqrt(P_ii P_jj) below `tol` (P_a square: an active part)."""
    P_a = np.asarray(P_a, dtype=float)
    d = np.abs(np.diag(P_a))
    a = float(np.max(np.abs(P_a - P_a.T) / np.sqrt(np.outer(d, d)))) if d.all() else float(np.abs(P_a - P_a.T).max())
    assert a < tol, f"{what}asymmetry: correlation-scaled max |P - P^T| = {a:.3e} exceeds {tol:g}"


def assert_filter_close(mu, P, om, oP, observed, mean0=None, diag0=None, tol=1e-9, what="", corr_tol=None):
    """Compare the state (mu, P) with the reference (om, oP) piece by piece (module docstring); returns {piece: error}.

    `observed`: landmark indices the stream observed (observed_landmarks).  `om` / `oP` may cover only a leading part of
    the state that holds the pose and every observed landmark (the oracle run on the active part of a block-diagonal start,
    a closed system): only the active indices are read.  `mean0` / `diag0`: the block-diagonal start; given, every landmark
    outside `observed` must come back exactly as it started, with exactly zero cross terms.  `corr_tol`: the bound of
    the per-entry maxima corr_max and mean_landmarks where it differs from `tol` (PATH_CORR_TOL between two GPU paths)."""
    mu, P = np.asarray(mu), np.asarray(P)
    n = len(mu)
    assert P.shape == (n, n), f"{what}covariance of shape {P.shape} for a mean of {n}"
    act = np.concatenate([np.arange(3), landmark_rows(observed)]).astype(np.int64)
    assert act.max() < len(om) and act.max() < np.asarray(oP).shape[0], f"{what}reference does not cover the active part"
    P_a = P[np.ix_(act, act)]
    assert_symmetric(P_a, tol, what)
    err = active_errors(mu[act], P_a, np.asarray(om)[act], np.asarray(oP)[np.ix_(act, act)])
    check_errors(err, tol, what, corr_tol)
    if mean0 is not None or diag0 is not None:
        rest = np.setdiff1d(np.arange(3, n), act)
        if len(rest):
            if mean0 is not None:
                bad = np.flatnonzero(mu[rest] != np.asarray(mean0)[rest])
                assert not len(bad), f"{what}never-observed mean: {len(bad)} entries differ from the start (first at {rest[bad[0]]})"
            if diag0 is not None:
                bad = np.flatnonzero(np.diag(P)[rest] != np.asarray(diag0)[rest])
                assert not len(bad), (f"{what}never-observed variance: {len(bad)} entries differ from the start "
                                      f"(first at {rest[bad[0]]})")
            # their rows (against everything) and their columns (against the active part): zero but for the diagonal,
            # in chunks of rows (at N = 8000 P is 2 GB)
            assert not P[np.ix_(act, rest)].any(), f"{what}never-observed cross terms: non-zero in the active rows"
            for r0 in range(0, len(rest), 512):
                r = rest[r0:r0 + 512]
                rows = P[r]
                rows[np.arange(len(r)), r] = 0.0
                nz = np.count_nonzero(rows)
                assert nz == 0, f"{what}never-observed cross terms: {nz} non-zero entries in rows {r[0]}..{r[-1]}"
    return err


UPDATE_PIECES = PIECES + ("touched_block", "touched_mean", "touched_cross")


def landmark_classes(before_P, touched, init_var):
    """The landmarks of a state by what an update finds: (active, first, rest) -- variance below `init_var` in `before_P`
    (observed, or fixed, at some time), never observed and named in `touched`, never observed and not named."""
    d = np.diag(np.asarray(before_P))
    N = (len(d) - 3) // 2
    never = ~((d[3::2] < init_var) & (d[4::2] < init_var))
    named = np.zeros(N, dtype=bool)
    named[[int(l) for l in touched if int(l) >= 0]] = True
    lms = np.arange(N)
    return lms[~never], lms[never & named], lms[never & ~named]


def active_of(P, init_var):
    """The landmarks of a reference covariance that have been observed (fixed, or tied in) at some time."""
    return landmark_classes(P, [], init_var)[0]


def assert_update_close(got, want, before, touched, init_var, tol, what="", entry_tol=None, first_cross_tol=None):
    """ONE update (direct or linear) applied to a known state: `got` = (mean, P) after the call, `want` the reference's
    result, `before` the state the call found, `touched` the landmarks the call names.  The landmarks fall into three
    classes by `before` (landmark_classes), each judged on its own scale; returns {piece: measured value}.

    active before the call, and the pose: the pieces of `assert_filter_close` (PIECES) of `got` against `want`, each below
      `tol`; the per-entry maxima corr_max and mean_landmarks below `entry_tol` where given (a dense H that ties a
      never-observed landmark in: its 1e4 cancels inside entries of the active part too).
    first touched by this call (never observed before): own 2 x 2 block within 32 eps init_var absolutely (the update forms
      v - v^2 / (v + R)), mean within 1e-9 relatively (`touched_block`, `touched_mean`); their cross terms with everything
      else (`touched_cross`): with `first_cross_tol` None (a direct fix) bit-equal to `before` and exactly zero, else
      max |dP_ij| / sqrt(wP_ii wP_jj) against the active part and among themselves below it, exactly zero against the rest.
    untouched and never observed: mean, variance and whole rows of P bit-equal to `before`, cross terms exactly zero.
    `got`'s covariance must be exactly symmetric."""
    mu, P = np.asarray(got[0]), np.asarray(got[1])
    wm, wP = np.asarray(want[0]), np.asarray(want[1])
    bm, bP = np.asarray(before[0]), np.asarray(before[1])
    n = len(mu)
    assert P.shape == (n, n) and wP.shape == (n, n) and bP.shape == (n, n) and len(wm) == n and len(bm) == n, \
        f"{what}shapes differ: got {P.shape}, want {wP.shape}, before {bP.shape}"
    for r0 in range(0, n, 512):                        # (in chunks of rows: the panel cases hold 136 MB)
        assert np.array_equal(P[r0:r0 + 512], P[:, r0:r0 + 512].T), f"{what}asymmetry: P != P^T in rows {r0}..{r0 + 511}"
    active, first, rest = landmark_classes(bP, touched, init_var)
    act = np.concatenate([np.arange(3), landmark_rows(active)]).astype(np.int64)
    err = active_errors(mu[act], P[np.ix_(act, act)], wm[act], wP[np.ix_(act, act)])
    check_errors(err, tol, what, entry_tol)
    frows, rrows = landmark_rows(first), landmark_rows(rest)
    if len(first):
        eps_v = 32 * np.finfo(float).eps * init_var
        blk = max(float(np.abs(P[a:a + 2, a:a + 2] - wP[a:a + 2, a:a + 2]).max()) for a in 3 + 2 * first)
        err["touched_block"] = blk
        assert blk <= eps_v, f"{what}touched_block: {blk:.3e} exceeds 32 eps init_var = {eps_v:.3e}"
        dm = max(float(np.abs(mu[a:a + 2] - wm[a:a + 2]).max() / max(1.0, np.abs(wm[a:a + 2]).max())) for a in 3 + 2 * first)
        err["touched_mean"] = dm
        assert dm <= 1e-9, f"{what}touched_mean: {dm:.3e} exceeds 1e-9"
        own = np.zeros((len(frows), n), dtype=bool)    # a first-touched landmark's own 2 x 2 block, in its two rows
        for i, r in enumerate(frows):
            a = 3 + 2 * ((r - 3) // 2)
            own[i, a:a + 2] = True
        rows = P[frows]
        if first_cross_tol is None:
            same = np.array_equal(rows[~own], bP[frows][~own])
            err["touched_cross"] = float(np.abs(rows[~own]).max())
            assert same and err["touched_cross"] == 0.0, \
                f"{what}touched_cross: a direct fix of a never-observed landmark moved its cross terms (max {err['touched_cross']:.3e})"
        else:
            cols = np.concatenate([act, frows])
            d = np.sqrt(np.outer(np.diag(wP)[frows], np.diag(wP)[cols]))
            dev = np.abs(rows[:, cols] - wP[np.ix_(frows, cols)]) / d
            dev[own[:, cols]] = 0.0
            err["touched_cross"] = float(dev.max())
            assert err["touched_cross"] < first_cross_tol and err["touched_cross"] < REL_TOL, \
                f"{what}touched_cross: {err['touched_cross']:.3e} exceeds {first_cross_tol:g}"
            assert not rows[:, rrows].any(), f"{what}touched_cross: non-zero against never-observed landmarks"
    if len(rest):
        bad = np.flatnonzero(mu[rrows] != bm[rrows])
        assert not len(bad), f"{what}never-observed mean: {len(bad)} entries differ from before the call (first at {rrows[bad[0]]})"
        bad = np.flatnonzero(np.diag(P)[rrows] != np.diag(bP)[rrows])
        assert not len(bad), f"{what}never-observed variance: {len(bad)} entries differ from before the call (first at {rrows[bad[0]]})"
        assert not P[np.ix_(act, rrows)].any(), f"{what}never-observed cross terms: non-zero in the active rows"
        for r0 in range(0, len(rrows), 512):
            r = rrows[r0:r0 + 512]
            rows = P[r]
            assert np.array_equal(rows, bP[r]), f"{what}never-observed rows {r[0]}..{r[-1]} differ from before the call"
            rows[np.arange(len(r)), r] = 0.0
            nz = np.count_nonzero(rows)
            assert nz == 0, f"{what}never-observed cross terms: {nz} non-zero entries in rows {r[0]}..{r[-1]}"
    return err


STATE_PIECES = PIECES + ("loose_block", "loose_mean", "loose_cross")


def loose_landmarks(P, init_var):
    """(loose, informed) landmarks of a state by the state itself: loose = both variances at or above half of `init_var`
    (never informed by anything: a prior), informed = the rest."""
    d = np.diag(np.asarray(P))
    is_loose = (d[3::2] >= 0.5 * init_var) & (d[4::2] >= 0.5 * init_var)
    lms = np.arange(len(is_loose))
    return lms[is_loose], lms[~is_loose]


def state_errors(got, want, init_var):
    """What `assert_state_close` measures, without judging it: (mean, P) `got` against (mean, P) `want`, the landmarks classed
    by `want`.  -> {piece: value}: PIECES on the pose and the informed landmarks; for the loose ones loose_block (own 2 x 2
    blocks, absolute), loose_mean (relative to max(1, |mean|)), loose_cross (max |dP_ij| / sqrt(wP_ii wP_jj) over their rows,
    the own block apart, where `want` is not exactly zero) and loose_zeros (entries of those rows that are exactly zero in
    `want` and not in `got`)."""
    mu, P = np.asarray(got[0], dtype=float), np.asarray(got[1], dtype=float)
    wm, wP = np.asarray(want[0], dtype=float), np.asarray(want[1], dtype=float)
    loose, informed = loose_landmarks(wP, init_var)
    act = np.concatenate([np.arange(3), landmark_rows(informed)]).astype(np.int64)
    err = active_errors(mu[act], P[np.ix_(act, act)], wm[act], wP[np.ix_(act, act)])
    if len(loose):
        rows = landmark_rows(loose)
        err["loose_block"] = max(float(np.abs(P[a:a + 2, a:a + 2] - wP[a:a + 2, a:a + 2]).max()) for a in 3 + 2 * loose)
        err["loose_mean"] = max(float(np.abs(mu[a:a + 2] - wm[a:a + 2]).max() / max(1.0, np.abs(wm[a:a + 2]).max()))
                                for a in 3 + 2 * loose)
        g, w = P[rows].copy(), wP[rows].copy()
        for i, r in enumerate(rows):                      # (the own block is judged above)
            a = 3 + 2 * ((r - 3) // 2)
            g[i, a:a + 2] = w[i, a:a + 2] = 0.0
        zero = w == 0.0
        err["loose_zeros"] = int(np.count_nonzero(g[zero]))
        dev = np.abs(g - w) / np.sqrt(np.outer(np.diag(wP)[rows], np.diag(wP)))
        err["loose_cross"] = float(dev[~zero].max()) if (~zero).any() else 0.0
    return err


def assert_state_close(got, model_state, init_var, tol=1e-9, entry_tol=None, what=""):
    """A WHOLE state after any sequence of calls: `got` = (mean, P, tag index, flags) of a filter against `model_state` =
    (mean, P, tag index) of the dense model fed the same calls.  The landmarks are classed by the model's state, not by
    history (loose_landmarks); returns {piece: measured value}.

    informed landmarks, and the pose: the six PIECES of `active_errors`, each below `tol` (and the 1e-6 bar);
    loose landmarks: own 2 x 2 block within 32 eps init_var absolutely, mean within 1e-9 relatively (loose_block, loose_mean:
      `assert_update_close`'s rule for a first-touched landmark); cross terms (loose_cross) exactly zero wherever the model's
      entry is exactly zero, elsewhere max |dP_ij| / sqrt(P_ii P_jj) below `entry_tol` (a transform with a covariance, a
      predict_dense: a prior of 1e4 carries correlations, and every later update cancels against it);
    the whole state: P exactly symmetric, size and tag index equal to the model's, flags 0."""
    mu, P, tags, flags = got
    wm, wP, wtags = model_state
    mu, P = np.asarray(mu), np.asarray(P)
    n = len(wm)
    assert len(mu) == n and P.shape == (n, n), f"{what}size: a state of {len(mu)} ({P.shape}) where the model has {n}"
    assert flags == 0, f"{what}flags: {flags:#x}"
    assert dict(tags) == dict(wtags), f"{what}tags: tag index {dict(tags)} where the model has {dict(wtags)}"
    assert np.array_equal(P, P.T), f"{what}asymmetry: P != P^T"
    err = state_errors((mu, P), (wm, wP), init_var)
    check_errors(err, tol, what)
    if "loose_block" in err:
        eps_v = 32 * np.finfo(float).eps * init_var
        assert err["loose_block"] <= eps_v, f"{what}loose_block: {err['loose_block']:.3e} exceeds 32 eps init_var = {eps_v:.3e}"
        assert err["loose_mean"] <= 1e-9, f"{what}loose_mean: {err['loose_mean']:.3e} exceeds 1e-9"
        assert err["loose_zeros"] == 0, f"{what}loose_cross: {err['loose_zeros']} entries non-zero where the model holds exact zeros"
        if err["loose_cross"] > 0.0:
            assert entry_tol is not None and err["loose_cross"] < entry_tol and err["loose_cross"] < REL_TOL, \
                f"{what}loose_cross: {err['loose_cross']:.3e} exceeds " + ("no bound given" if entry_tol is None else f"{entry_tol:g}")
    return err


def fmt_state(err):
    return " ".join(f"{k}={err[k]:.2e}" for k in STATE_PIECES if k in err)


def fmt_update(err):
    return " ".join(f"{k}={err[k]:.2e}" for k in UPDATE_PIECES if k in err)


def assert_marginals_close(pose, lms, oP, observed, diag0=None, tol=1e-9, what=""):
    """`EkfSlam.marginals(b)` -> (pose (3, 3), landmarks (N, 2, 2)) against the reference covariance: the pose block and
    the observed landmarks' 2 x 2 blocks (relative Frobenius), the never-observed ones bit-equal to the start (`diag0`)."""
    observed = np.asarray(observed, dtype=np.int64)
    r = 3 + 2 * observed
    ref = np.stack([np.stack([oP[r, r], oP[r, r + 1]], -1), np.stack([oP[r + 1, r], oP[r + 1, r + 1]], -1)], -2)
    err = {"pose": _rel(pose, oP[:3, :3]), "landmarks": _rel(lms[observed], ref)}
    check_errors(err, tol, what + "marginals ")
    if diag0 is not None:
        rest = np.setdiff1d(np.arange(len(lms)), observed)
        d = np.asarray(diag0)
        want = np.zeros((len(rest), 2, 2))
        want[:, 0, 0], want[:, 1, 1] = d[3 + 2 * rest], d[4 + 2 * rest]
        assert np.array_equal(lms[rest], want), f"{what}marginals of never-observed landmarks differ from the start"
    return err


def marginal_blocks(P):
    """(pose (3, 3), landmarks (N, 2, 2)): the diagonal blocks of a covariance, as `EkfSlam.marginals(b)` returns them."""
    P = np.asarray(P)
    r = np.arange(3, P.shape[0], 2)
    return P[:3, :3].copy(), np.stack([np.stack([P[r, r], P[r, r + 1]], -1), np.stack([P[r + 1, r], P[r + 1, r + 1]], -1)], -2)


def marginal_errors(pose, lms, wP, init_var):
    """`EkfSlam.marginals(b)` against a dense model's covariance `wP`, the landmarks classed by the model as `loose_landmarks`
    does: pose and the informed landmarks' blocks by relative Frobenius norm, the loose ones' absolutely (loose_block)."""
    wpose, wlms = marginal_blocks(np.asarray(wP, dtype=float))
    loose, informed = loose_landmarks(wP, init_var)
    err = {"pose": _rel(pose, wpose)}
    if len(informed):
        err["landmarks"] = _rel(np.asarray(lms, dtype=float)[informed], wlms[informed])
    if len(loose):
        err["loose_block"] = float(np.abs(np.asarray(lms, dtype=float)[loose] - wlms[loose]).max())
    return err


def assert_marginal_blocks_close(pose, lms, wP, init_var, tol=1e-9, what=""):
    """`assert_state_close`'s rule on the diagonal blocks alone: as many landmark blocks as the model has landmarks, pose and
    informed blocks below `tol` (and the 1e-6 bar), loose blocks within 32 eps init_var; returns {piece: measured value}."""
    N = (np.asarray(wP).shape[0] - 3) // 2
    assert np.shape(pose) == (3, 3) and np.shape(lms) == (N, 2, 2), \
        f"{what}marginals count: {np.shape(lms)[0]} landmark blocks where the model has {N}"
    err = marginal_errors(pose, lms, wP, init_var)
    check_errors(err, tol, what + "marginals ")
    if "loose_block" in err:
        eps_v = 32 * np.finfo(float).eps * init_var
        assert err["loose_block"] <= eps_v, f"{what}marginals loose_block: {err['loose_block']:.3e} exceeds 32 eps init_var = {eps_v:.3e}"
    return err


def fmt(err):
    return " ".join(f"{k}={err[k]:.2e}" for k in PIECES if k in err)
