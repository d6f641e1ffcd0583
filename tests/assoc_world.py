"""Shared by the association tests (tests/test_associate_cpu.py, tests/test_gpu_associate.py): the NumPy reference of the
likelihood scores, the separable grid worlds, and a dense unlabelled EKF loop on the oracle."""
import numpy as np

from oracle import ekf_oracle as orc

ACCEPT = 9.21        # chi-square quantile, 2 degrees of freedom, 0.99
CREATE = 18.42       # ... 0.9999
WORLDS = {"4x4": (4, 0.6, 80, 4), "5x5": (5, 0.5, 100, 5), "6x6": (6, 0.5, 90, 8)}   # side, spacing, steps, m
SEEDS = (0, 1, 2)
# check_query: NIS relative 1e-9 cond_2(S_ref), ln det S absolute 2e-9 cond_2(S_ref) (tests/test_gpu_associate.py has the reasons)
NIS_TOL, LOGDET_TOL = 1e-9, 2e-9
TOTALS = {"entries": 0, "left_out": 0, "obs": 0, "excused": 0}


def world_cfg():
    return orc.EkfConfig(motion_sigma=0.02, meas_sigma=0.03)


def ref_scores(mu, P, ranges, bearings, qd):
    """Every landmark of the state (mu, P) against every observation: NIS (m, N), ln det S (N,), cond_2(S) (N,) and the
    unwrapped bearing residual (m, N).  The formula of the issue: H5 and the innovation as oracle.innovation_and_h5, the joint
    5 x 5 block of (pose, landmark), S = H5 P5 H5^T + diag(qd)."""
    N = (len(mu) - 3) // 2
    m = len(ranges)
    nis, raw = np.full((m, N), np.nan), np.full((m, N), np.nan)
    logdet, cond = np.full(N, np.nan), np.full(N, np.nan)
    for l in range(N):
        i = 3 + 2 * l
        sel = [0, 1, 2, i, i + 1]
        P5 = P[np.ix_(sel, sel)]
        _, h5 = orc.innovation_and_h5(mu[:3], mu[i:i + 2], 0.0, 0.0)
        S = h5 @ P5 @ h5.T + np.diag(qd)
        sign, logdet[l] = np.linalg.slogdet(S)
        if not sign > 0:
            logdet[l] = np.nan
        cond[l] = np.linalg.cond(S)
        d = mu[i:i + 2] - mu[:2]
        for q in range(m):
            y, _ = orc.innovation_and_h5(mu[:3], mu[i:i + 2], ranges[q], bearings[q])
            nis[q, l] = y @ np.linalg.solve(S, y)
            raw[q, l] = bearings[q] - (np.arctan2(d[1], d[0]) - mu[2])
    return nis, logdet, cond, raw


def check_query(f, state, zr, zb, m=None, meas_sigma=None, what="", res=None, totals=None):
    """f.associate(full=True) of the whole bank against the NumPy reference on the reference state: `state(b)` -> (mean,
    covariance) of trajectory b, called AFTER the query (a download, or a dense model's state).  Counts what it leaves out or
    excuses into `totals` (default: TOTALS).  Returns the query's result and the reference's cond(S) per trajectory."""
    totals = TOTALS if totals is None else totals
    a = f.associate(zr, zb, m, full=True) if res is None else res
    B, S = a.cand.shape[:2]
    R, Bg, mm = f._unlabelled(zr, zb, m)
    sig = np.broadcast_to(f.config.meas_sigma if meas_sigma is None else meas_sigma, (B,))
    conds = []
    for b in range(B):
        mu, P = state(b)
        N, mb = (len(mu) - 3) // 2, int(mm[b])
        nis, logdet, cond, raw = ref_scores(mu, P, R[b, :mb], Bg[b, :mb], np.array([sig[b] ** 2] * 2))
        conds.append(cond)
        assert np.isnan(a.all_nis[b, :, N:]).all() and np.isnan(a.all_logdet[b, :, N:]).all(), what
        assert np.isnan(a.all_nis[b, mb:]).all() and (a.cand[b, mb:] == -1).all() and np.isnan(a.min_nis[b, mb:]).all(), what
        assert np.isnan(a.nis[b, mb:]).all() and np.isnan(a.logdet[b, mb:]).all(), what
        if mb == 0:
            continue
        if N == 0:
            assert (a.cand[b] == -1).all() and np.isnan(a.nis[b]).all() and np.isnan(a.min_nis[b]).all(), what
            continue
        got_nis, got_ld = a.all_nis[b, :mb, :N], a.all_logdet[b, :mb, :N]
        near = np.abs(np.mod(raw, 2 * np.pi) - np.pi) < 1e-9          # the wrap may fall either way there
        totals["entries"] += near.size
        totals["left_out"] += int(near.sum())
        assert near.sum() <= 1e-3 * near.size, what
        e_nis = np.abs(got_nis - nis) / np.abs(nis)
        e_ld = np.abs(got_ld - logdet[None, :])
        print(f"{what}trajectory {b}: N={N} m={mb} NIS rel err / cond max {np.nanmax(np.where(near, 0, e_nis / cond)):.2e} "
              f"logdet abs err / cond max {np.nanmax(e_ld / cond):.2e} cond max {cond.max():.2e}")
        assert not np.isnan(got_nis).any() and not np.isnan(got_ld).any(), what
        assert (np.where(near, 0.0, e_nis) <= NIS_TOL * cond[None, :]).all(), what
        assert (e_ld <= LOGDET_TOL * cond[None, :]).all(), what
        # the candidates: the query's own numbers first (same lane, same bits), then against the reference's order
        gd = got_nis + got_ld
        for q in range(mb):
            for c in range(min(2, N)):
                j = a.cand[b, q, c]
                assert 0 <= j < N and a.nis[b, q, c] == got_nis[q, j] and a.logdet[b, q, c] == got_ld[q, j], what
            order = np.argsort(gd[q], kind="stable")
            assert list(a.cand[b, q, :min(2, N)]) == list(order[:2]), what   # ascending d, ties to the lower index
            if N == 1:
                assert a.cand[b, q, 1] == -1 and np.isnan(a.nis[b, q, 1])
            assert a.min_nis[b, q] == got_nis[q].min(), what
        tol_d = NIS_TOL * cond[None, :] * np.abs(nis) + LOGDET_TOL * cond[None, :]
        d_ref = nis + logdet[None, :]
        for q in range(mb):
            totals["obs"] += 1
            order = np.argsort(d_ref[q], kind="stable")
            clear = all(d_ref[q, order[r + 1]] - d_ref[q, order[r]] > tol_d[q, order[r + 1]] + tol_d[q, order[r]]
                        for r in range(min(2, N - 1)))
            if not clear or near[q].any():
                totals["excused"] += 1
                continue
            assert list(a.cand[b, q, :min(2, N)]) == list(order[:2]), (what, b, q)
    return a, conds


def ref_candidates(nis, logdet):
    """(cand (m, 2), cand_nis (m, 2), min_nis (m,), sorted scores (m, N)) of the reference scores: ascending d = NIS + ln det S,
    ties to the lower index, NaN never wins; -1 / NaN where there is no candidate."""
    m, N = nis.shape
    d = nis + logdet[None, :]
    cand = np.full((m, 2), -1, dtype=np.int64)
    cnis = np.full((m, 2), np.nan)
    mn = np.full(m, np.nan)
    ds = np.full((m, N), np.nan)
    for q in range(m):
        ok = np.flatnonzero(~np.isnan(d[q]))
        order = ok[np.argsort(d[q, ok], kind="stable")]
        ds[q, :len(order)] = d[q, order]
        for c in range(min(2, len(order))):
            cand[q, c] = order[c]
            cnis[q, c] = nis[q, order[c]]
        if np.any(~np.isnan(nis[q])):
            mn[q] = np.nanmin(nis[q])
    return cand, cnis, mn, ds


def make_world(name, seed):
    """(landmarks (N, 2), steps, m) of the grid world `name`: side x side landmarks `spacing` apart, centred at (0.13, 0.29),
    each coordinate jittered uniformly by +-0.05."""
    side, spacing, steps, m = WORLDS[name]
    rng = np.random.default_rng(seed)
    g = (np.arange(side) - (side - 1) / 2.0) * spacing
    lm = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) + np.array([0.13, 0.29])
    lm = lm + rng.uniform(-0.05, 0.05, lm.shape)
    return lm, steps, m


def make_run(name, seed):
    """The inputs of a run through the world: per step (lin, ang), the true labels (m,) and the observations (ranges, bearings)
    of the landmarks (m k + arange(m)) % N, seen from the true pose with noise 0.01 on the landmark's robot-frame coordinates.
    The true pose follows the motion model from the origin: lin = 0.004, ang = 0.02, every 10th step ang = 0.005."""
    lm, steps, m = make_world(name, seed)
    N = len(lm)
    rng = np.random.default_rng(1000 + seed)
    cfg = world_cfg()
    pose = np.zeros(3)
    out = []
    for k in range(steps):
        lin, ang = 0.004, (0.005 if k % 10 == 9 else 0.02)
        pose, _ = orc.motion_model(pose, lin, ang, cfg)
        vis = (m * k + np.arange(m)) % N
        d = lm[vis] - pose[:2]
        c, s = np.cos(pose[2]), np.sin(pose[2])
        xr = c * d[:, 0] + s * d[:, 1] + rng.normal(0.0, 0.01, m)
        yr = -s * d[:, 0] + c * d[:, 1] + rng.normal(0.0, 0.01, m)
        out.append((lin, ang, vis, np.hypot(xr, yr), np.arctan2(yr, xr)))
    return lm, out


def dense_unlabelled_run(name, seed, resolve):
    """The unlabelled loop on the dense oracle: predict_dense, scores by `ref_scores`, `resolve` (frontend.resolve_associations),
    augment for the new observations (world position from the predicted pose), update_dense in observation order.  Returns
    what the test asserts on: wrong and dropped observations, how often each world landmark was created, the smallest
    runner-up margin in d, and the final (mean, cov)."""
    lm, run = make_run(name, seed)
    cfg = world_cfg()
    mean, cov = np.zeros(3), np.eye(3) * cfg.motion_sigma
    created = np.zeros(len(lm), dtype=int)
    world_of = []                                        # filter landmark -> world landmark
    wrong = dropped = 0
    margin = np.inf
    for lin, ang, vis, zr, zb in run:
        mean, cov = orc.predict_dense(mean, cov, lin, ang, cfg)
        nis, logdet, _, _ = ref_scores(mean, cov, zr, zb, cfg.meas_noise_diag())
        cand, cnis, mn, ds = ref_candidates(nis, logdet)
        assign, new_obs, drop = resolve(cand, cnis, mn, ACCEPT, CREATE)
        dropped += len(drop)
        for q in np.flatnonzero(assign >= 0):
            wrong += int(world_of[assign[q]] != vis[q])
            if len(world_of) >= 2:
                margin = min(margin, ds[q, 1] - ds[q, 0])
        if new_obs:
            n_lm = len(world_of)
            pos = {}
            for t, q in enumerate(new_obs):
                pos[n_lm + t] = (mean[0] + zr[q] * np.cos(zb[q] + mean[2]), mean[1] + zr[q] * np.sin(zb[q] + mean[2]))
                assign[q] = n_lm + t
                created[vis[q]] += 1
                world_of.append(int(vis[q]))
            mean, cov = orc.augment(mean, cov, len(world_of), pos, cfg)
        keep = np.flatnonzero(assign >= 0)
        mean, cov = orc.update_dense(mean, cov, assign[keep], zr[keep], zb[keep], cfg)
    return dict(wrong=wrong, dropped=dropped, created=created, margin=margin, mean=mean, cov=cov)
