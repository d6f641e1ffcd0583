"""A CPU backend for slam_duckietown_amd.replay built from the oracle: what the replay driver's and the node adapter's tests
run the events through where there is no GPU."""
import numpy as np

from oracle import ekf_oracle as orc


class OracleBackend:
    """Test double with the backend protocol of slam_duckietown_amd.replay (CPU, oracle arithmetic)."""

    def __init__(self):
        self.cfg = orc.EkfConfig()
        self.mean, self.cov = np.zeros(3), np.eye(3) * 0.1

    def set_state(self, mean, cov):
        self.mean, self.cov = np.array(mean, dtype=float), np.array(cov, dtype=float)

    def pose(self):
        return self.mean[:3]

    def state(self):
        return self.mean, self.cov

    def step(self, ang, lin, detections, tag_index):
        self.mean, self.cov, tags = orc.ekf_pose_estimation_dense(ang, lin, self.mean, self.cov, 0.7, detections,
                                                                  tag_index, self.cfg)
        return tags

    def close(self):
        pass
