"""What tests/parity_blocks.py catches that the whole-matrix check does not (no GPU).

Oracle states of the streams the GPU parity tests use from a block-diagonal start -- config 3 (N = 2000, 12 steps),
config 5's active part (12 steps inside 3000 of 8000 landmarks) and config 2 (N = 500, 50 steps) -- perturbed the way a
subtly wrong kernel would perturb them.  At config 3 and 5 every perturbation below passes the old check
(`rel_fro < 1e-9` on the whole mean and matrix) and each one fails the block-wise helper, naming its piece.
"""
import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import parity_blocks as pb

TIGHT = 1e-9


def old_close(a, b, tol=TIGHT):
    return orc.rel_fro(a, b) < tol


def _oracle(N, steps, tid, remap=None):
    """-> oracle mean and covariance after `steps` steps from the block-diagonal start, the landmarks observed, the start.
    With `remap` (config 5's observations inside the first 3000 landmarks) on the active part only: a closed system."""
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, 8, tid)
    if remap is not None:
        idx = remap(idx)
    obs = pb.observed_landmarks(idx)
    top = 3 + 2 * (int(obs.max()) + 1) if remap is not None else len(mean0)
    cfg = orc.EkfConfig()
    om, oP = mean0[:top].copy(), np.diag(diag0[:top])
    for k in range(steps):
        om, oP = orc.ekf_step_structured(om, oP, lin[k], ang[k], idx[k], zr[k], zb[k], cfg)
    return om, oP, obs, mean0[:top], diag0[:top]


STREAMS = {"config3_n2000": lambda: _oracle(2000, 12, 3),
           "config5_n8000_active": lambda: _oracle(8000, 12, 9, lambda i: (i * 37 + 5) % 3000),
           "config2_n500": lambda: _oracle(500, 50, 0)}
# where the old whole-matrix check is blind to every perturbation below (rel_fro 4e-10 .. 6e-10 at most)
OLD_BLIND = ("config3_n2000", "config5_n8000_active")


@pytest.fixture(scope="module", params=list(STREAMS))
def state(request):
    om, oP, obs, mean0, diag0 = STREAMS[request.param]()
    assert (3 + 2 * (int(obs.max()) + 1) < len(om)) or len(obs) < (len(om) - 3) // 2   # never-observed landmarks exist
    return request.param, om, oP, obs, mean0, diag0


def _helper_fails(mu, P, om, oP, obs, mean0, diag0, piece):
    with pytest.raises(AssertionError, match=piece):
        pb.assert_filter_close(mu, P, om, oP, obs, mean0=mean0, diag0=diag0, tol=TIGHT)


def test_exact_state_passes(state):
    _, om, oP, obs, mean0, diag0 = state
    err = pb.assert_filter_close(om.copy(), oP.copy(), om, oP, obs, mean0=mean0, diag0=diag0)
    assert set(err) == set(pb.PIECES) and max(err.values()) == 0.0


def test_observed_landmarks_of_variable_streams():
    idx = np.array([[[4, 9, 0]], [[7, 0, 0]], [[0, 0, 0]]])
    m = np.array([[2], [1], [0]])
    assert pb.observed_landmarks(idx, m).tolist() == [4, 7, 9]
    assert pb.observed_landmarks(idx).tolist() == [0, 4, 7, 9]
    assert pb.landmark_rows([0, 2]).tolist() == [3, 4, 7, 8]


def unobserved_row(om, obs):
    """The last state index of a never-observed landmark."""
    return int(np.setdiff1d(np.arange(3, len(om)), pb.landmark_rows(obs))[-1])


def _cov_perturbations(om, oP, obs):
    s = pb.landmark_rows(obs)
    out = {}
    P = oP.copy()
    P[:3, :3] *= 1.001                                                   # pose block 0.1 % off
    out["pose"] = (om, P)
    P = oP.copy()
    P[:3, s] *= 1.0001                                                   # pose-landmark cross terms 0.01 % off
    P[s, :3] *= 1.0001
    out["cross"] = (om, P)
    P = oP.copy()
    i, j = 0, s[len(s) // 2]                                             # ONE cross entry off by 1e-7 of its scale
    P[i, j] += 1e-7 * np.sqrt(oP[i, i] * oP[j, j])
    P[j, i] = P[i, j]
    out["corr_max"] = (om, P)
    mu = om.copy()
    mu[:3] *= 1 + 1e-7                                                   # the pose mean off by 1e-7
    out["mean_pose"] = (mu, oP)
    P = oP.copy()
    u = unobserved_row(om, obs)                                          # one entry of a never-observed row non-zero
    P[u, s[0]] = P[s[0], u] = 1e-12
    out["never-observed cross terms"] = (om, P)
    return out


@pytest.mark.parametrize("piece", ["pose", "cross", "corr_max", "mean_pose", "never-observed cross terms"])
def test_perturbation_passes_the_old_check_and_fails_the_helper(state, piece):
    name, om, oP, obs, mean0, diag0 = state
    mu, P = _cov_perturbations(om, oP, obs)[piece]
    if name in OLD_BLIND:
        assert old_close(mu, om) and old_close(P, oP), (orc.rel_fro(mu, om), orc.rel_fro(P, oP))
    _helper_fails(mu, P, om, oP, obs, mean0, diag0, piece)


def test_landmark_block_and_landmark_mean_are_checked(state):
    _, om, oP, obs, mean0, diag0 = state
    s = pb.landmark_rows(obs)
    P = oP.copy()
    P[np.ix_(s, s)] *= 1 + 1e-8
    _helper_fails(om, P, om, oP, obs, mean0, diag0, "landmarks")
    mu = om.copy()
    mu[s[-1]] += 1e-8 * np.sqrt(oP[s[-1], s[-1]])
    _helper_fails(mu, oP, om, oP, obs, mean0, diag0, "mean_landmarks")


def test_never_observed_mean_and_variance_must_be_the_start(state):
    _, om, oP, obs, mean0, diag0 = state
    u = unobserved_row(om, obs)
    mu = om.copy()
    mu[u] = np.nextafter(mu[u], np.inf)
    _helper_fails(mu, oP, om, oP, obs, mean0, diag0, "never-observed mean")
    P = oP.copy()
    P[u, u] = np.nextafter(P[u, u], 0)
    _helper_fails(om, P, om, oP, obs, mean0, diag0, "never-observed variance")


def test_asymmetric_covariance_is_refused(state):
    _, om, oP, obs, mean0, diag0 = state
    s = pb.landmark_rows(obs)
    P = oP.copy()
    P[1, s[0]] += 1e-7 * np.sqrt(oP[1, 1] * oP[s[0], s[0]])             # one side only
    _helper_fails(om, P, om, oP, obs, mean0, diag0, "asymmetry")


def test_marginals_helper(state):
    _, om, oP, obs, mean0, diag0 = state
    N = (len(om) - 3) // 2
    lms = np.zeros((N, 2, 2))
    for j in range(N):
        r = 3 + 2 * j
        lms[j] = oP[r:r + 2, r:r + 2]
    err = pb.assert_marginals_close(oP[:3, :3].copy(), lms, oP, obs, diag0=diag0)
    assert max(err.values()) == 0.0
    pose = oP[:3, :3] * 1.001
    with pytest.raises(AssertionError, match="marginals pose"):
        pb.assert_marginals_close(pose, lms, oP, obs, diag0=diag0)
    bad = lms.copy()
    bad[(unobserved_row(om, obs) - 3) // 2, 0, 1] = 1e-12
    with pytest.raises(AssertionError, match="never-observed"):
        pb.assert_marginals_close(oP[:3, :3], bad, oP, obs, diag0=diag0)
