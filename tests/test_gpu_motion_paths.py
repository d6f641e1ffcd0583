"""GPU: one motion model.  Every kernel that predicts calls motion_model (csrc/ekf_devfn.h), so predict-only steps -- no
observation, nothing for a path's own update arithmetic to add -- leave the SAME pose-mean bits on every path:

  small         step() on the small-state path                                  (ekf_small.hip small_step)
  general       step() with "small_state" 0                                     (ekf_kernels.hip solve_body)
  stream        an uploaded stream through stream_run, "small_state" 0          (ekf_solve_cad_body.inc, the chain's motion())
  localize      localize()                                                      (ekf_loc_chain.h loc_solve_body, k_loc_solve)
  run_localize  the uploaded stream through run_localize                        (the same, read from the stream)
  hypotheses    a hypothesis bank of K = 1 per trajectory                       (the same, k_hyp_solve)

The motions: ang of 0, +-5e-3 and +-2e-2 (either side of the 1e-2 arc threshold), lin = 0, and turns that carry theta over pi
(the wrap), from a start at theta = 3.09; under the default config and in linear mode (enable_circular_interpolation off, no
wrap); 20 landmarks (n = 43), batch 1 and 3 with a different start and a different order of the motions per trajectory.  Compared:
the pose mean behind EVERY step (the pose log's rows; the bank's poses are downloaded step by step), np.array_equal.  No path is
left out of the equality: on the commit before the shared function all six already agreed, bit for bit
(profiles/shared_device_arithmetic.txt) -- four copies of the same text.
"""
import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.gpu_support import sd  # noqa: F401

pytestmark = pytest.mark.gpu

N_MAX = 43
MOT = [(0.05, 0.0), (0.05, 5e-3), (0.04, -5e-3), (0.05, 2e-2), (0.03, -2e-2), (0.0, 2e-2), (0.0, 0.0), (0.06, 2e-2), (0.05, 2e-2),
       (0.0, -5e-3), (0.05, 2e-2), (0.02, 2e-2)]
K = len(MOT)
TH0 = 3.09
PATHS = ("small", "general", "stream", "localize", "run_localize", "hypotheses")


def motions(B):
    """(lin, ang), each (K, B): trajectory b takes the motions in an order of its own."""
    order = [[MOT[(k + 5 * b) % K] for b in range(B)] for k in range(K)]
    return np.array([[m[0] for m in row] for row in order]), np.array([[m[1] for m in row] for row in order])


def run(sd, path, cfg, B):
    """The pose means behind every step, (K, B, 3)."""
    lin, ang = motions(B)
    _rng, _lm, mean0, diag0 = orc.synthetic_world((N_MAX - 3) // 2, 3)
    none = np.zeros((B, 0))
    with sd.EkfSlam(N_MAX, batch=B, config=cfg) as f:
        if path in ("general", "stream"):
            f.set_option("small_state", 0)
        for b in range(B):
            m0 = mean0.copy()
            m0[:3] = 0.3 - 0.1 * b, -0.2 + 0.05 * b, TH0 - 0.02 * b
            f.set_state_diag(m0, diag0, b)
        if path == "hypotheses":
            out = np.empty((K, B, 3))
            for b in range(B):
                with f.hypotheses(1, b) as bank:
                    for k in range(K):
                        bank.step(lin[k, b], ang[k, b], [], [], [])
                        out[k, b] = bank.poses()[0][0]
            return out
        f.log_poses(K)
        if path in ("stream", "run_localize"):
            f.stream_upload(lin, ang, np.zeros((K, B, 1), dtype=np.int32), np.zeros((K, B, 1)), np.zeros((K, B, 1)),
                            np.zeros((K, B), dtype=np.int32))
            if path == "stream":
                f.stream_run(0, K)
            else:
                f.run_localize(0, K)
        else:
            call = f.localize if path == "localize" else f.step
            for k in range(K):
                call(lin[k], ang[k], none.astype(np.int32), none, none)
        small = sd.load_library().ekf_debug_small_launches(f._h)
        assert (small > 0) == (path == "small"), (path, small)
        tr = f.poses()
        assert tr.first == 0 and tr.mean.shape == (K, B, 3)
        assert np.array_equal(tr.mean[-1], np.stack([f.mean(b)[:3] for b in range(B)]))
        return tr.mean


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", ["default", "linear"])
def test_predict_only_steps_leave_the_same_pose_bits_on_every_path(sd, mode, B):
    cfg = sd.EkfConfig(enable_circular_interpolation=(mode == "default"))
    got = {p: run(sd, p, cfg, B) for p in PATHS}
    ref = got["small"]
    assert np.isfinite(ref).all()
    if mode == "default":
        assert (ref[..., 2] < -3.0).any() and (np.abs(ref[..., 2]) <= np.pi).all()      # theta went over pi and was wrapped
    else:
        assert (ref[..., 2] > np.pi).any()                                               # linear mode does not wrap (:409)
    for p in PATHS:
        differing = int((got[p] != ref).sum())
        print(f"{mode}, batch {B}, {p}: {differing} of {ref.size} pose-mean values differ from the small path's")
    for p in PATHS:
        assert np.array_equal(got[p], ref), p
