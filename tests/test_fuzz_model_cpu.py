"""CPU: the oracle model of tests/fuzz_model.py (what tests/test_gpu_fuzz_features.py compares the filter with) against the
oracle itself -- gate off, per-trajectory noise, removal, tag renumbering, the margin filter."""
import math

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from slam_duckietown_amd.frontend import remap_tag_index
from tests import fuzz_model as fm
from tests.gated_oracle import update_log


def start(N, seed, var=0.05):
    rng = np.random.default_rng(seed)
    _, lm, mean0, _ = orc.synthetic_world(N, seed)
    mean0 = mean0.copy()
    mean0[3:] = lm.ravel()
    cov = np.diag(np.concatenate([[0.1, 0.1, 0.1], np.full(2 * N, var)]))
    return rng, lm, mean0, cov


def observe(rng, tr, lm, m):
    """m landmarks measured from the model's own pose estimate (truth lm) + noise."""
    idx = rng.choice(len(lm), size=m, replace=False)
    d = lm[idx] - tr.mean[0:2]
    zr = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0, 0.03, m)
    zb = np.arctan2(d[:, 1], d[:, 0]) - tr.mean[2] + rng.normal(0, 0.03, m)
    return idx.astype(np.int32), zr, zb


def test_infinite_threshold_is_the_ungated_update():
    rng, lm, mean0, cov = start(30, 1)
    cfg = orc.EkfConfig()
    bank = fm.Bank([(mean0, cov)])
    bank.log_innovations(8)
    om, oP = mean0.copy(), cov.copy()
    rm, rP = mean0.copy(), cov.copy()
    for k in range(6):
        obs = observe(rng, bank.t[0], lm, 6)
        kept = bank.update([obs])
        assert len(kept[0][0]) == 6 and bank.dropped == 0                  # (gate off: nothing is ambiguous)
        om, oP, ys, Ss = update_log(om, oP, *obs, cfg)                     # the same arithmetic: bit for bit
        rm, rP = orc.update_dense(rm, rP, *obs, cfg)                       # the reference's form: to rounding
        assert np.array_equal(bank.t[0].mean, om) and np.array_equal(bank.t[0].cov, oP)
        assert orc.rel_fro(bank.t[0].mean, rm) < 1e-12 and orc.rel_fro(bank.t[0].cov, rP) < 1e-12
        idx, y, S, nis, rej = bank.log[k][0]
        assert np.array_equal(idx, obs[0]) and np.array_equal(y, ys) and np.array_equal(S, Ss) and not rej.any()
    assert bank.t[0].rejections == 0 and bank.log_steps == 6


def test_per_trajectory_config_is_the_oracle_with_that_config():
    rng, lm, mean0, cov = start(25, 2)
    bank = fm.Bank([(mean0, cov)] * 3)
    bank.set_noise(np.array([0.05, 0.1, 0.2]), np.array([0.3, 0.7, 1.1]))
    ms, qs = bank.noise()
    assert ms.tolist() == [0.05, 0.1, 0.2] and qs.tolist() == [0.3, 0.7, 1.1]
    bank.log_innovations(4)
    cfgs = [orc.EkfConfig(motion_sigma=a, meas_sigma=c) for a, c in zip(ms, qs)]
    ref = [(mean0.copy(), cov.copy()) for _ in range(3)]
    for k in range(5):
        lin, ang = np.full(3, 0.01), np.array([0.02, -0.1, 0.2])
        obs = [observe(rng, bank.t[b], lm, 5) for b in range(3)]
        bank.step(lin, ang, obs)
        for b in range(3):
            om, oP = orc.predict_dense(*ref[b], lin[b], ang[b], cfgs[b])
            ref[b] = update_log(om, oP, *obs[b], cfgs[b])[:2]
            assert orc.rel_fro(bank.t[b].mean, ref[b][0]) < 1e-12 and orc.rel_fro(bank.t[b].cov, ref[b][1]) < 1e-12
    assert sorted(bank.ring()) == [1, 2, 3, 4] and bank.log_steps == 5
    bank.predict(np.full(3, 0.01), np.zeros(3))                            # a lone prediction is no logged step
    assert bank.log_steps == 5
    bank.set_noise(None, 0.5)                                              # None: the handle's constant
    assert bank.noise()[0].tolist() == [0.1] * 3 and bank.noise()[1].tolist() == [0.5] * 3
    bank.set_noise()
    assert all(tr.cfg == orc.EkfConfig() for tr in bank.t)


def test_removal_then_stepping_is_stepping_the_deleted_state():
    rng, lm, mean0, cov = start(40, 3)
    cfg = orc.EkfConfig()
    bank = fm.Bank([(mean0, cov)])
    for _ in range(3):
        bank.step([0.01], [0.05], [observe(rng, bank.t[0], lm, 6)])
    before = bank.t[0].mean.copy(), bank.t[0].cov.copy()
    rm = [0, 7, 8, 39]
    o2n = bank.remove(rm, 0)
    rows = [3 + 2 * l + e for l in rm for e in (0, 1)]
    om, oP = np.delete(before[0], rows), np.delete(np.delete(before[1], rows, 0), rows, 1)
    assert np.array_equal(bank.t[0].mean, om) and np.array_equal(bank.t[0].cov, oP)
    assert o2n.tolist() == [-1 if j in rm else j - sum(r < j for r in rm) for j in range(40)]
    keep = np.setdiff1d(np.arange(40), rm)
    lm2 = lm[keep]
    for _ in range(3):
        obs = observe(rng, bank.t[0], lm2, 5)
        bank.step([0.01], [0.05], [obs])
        om, oP = orc.ekf_step_dense(om, oP, 0.01, 0.05, *obs, cfg)
        assert orc.rel_fro(bank.t[0].mean, om) < 1e-12 and orc.rel_fro(bank.t[0].cov, oP) < 1e-12


def test_tag_renumbering_agrees_with_the_front_end():
    rng = np.random.default_rng(4)
    bank = fm.Bank([(np.zeros(3), np.eye(3) * 0.1)] * 2)
    ids = [int(i) for i in rng.permutation(300)[:12]]
    new_xz = {i: (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.4, 1.1))) for i in ids}
    for w in (ids[:7], ids[5:12]):
        wins = [fm.window_of(rng, tr, w, new_xz, 2) for tr in bank.t]
        bank.window(np.full(2, 0.002), np.full(2, 0.01), wins)
    assert sorted(bank.t[0].tags) == sorted(ids) and sorted(bank.t[0].tags.values()) == list(range(12))
    before = dict(bank.t[0].tags)
    o2n = bank.remove([2, 3, 11], None)
    for tr in bank.t:
        assert tr.tags == remap_tag_index(before, o2n)
        assert sorted(tr.tags.values()) == list(range(9))
    gone = [t for t, j in before.items() if j == 3][0]
    wins = [fm.window_of(rng, tr, [gone, ids[0]], new_xz, 2) for tr in bank.t]
    bank.window(np.zeros(2), np.zeros(2), wins)
    assert bank.t[0].tags[gone] == 9 and bank.t[0].n_lm == 10             # seen again: a new landmark at the end


@pytest.mark.parametrize("g", [2.0, 6.0, 25.0])
def test_margin_filter_terminates_and_leaves_no_ambiguous_nis(g):
    rng, lm, mean0, cov = start(30, 5, var=0.02)
    bank = fm.Bank([(mean0, cov)] * 2)
    bank.set_noise(None, [0.05, 0.1])                                      # (small noise: many NIS near small thresholds)
    bank.set_nis_gate(g)
    bank.log_innovations(64)
    rejected = 0
    for k in range(8):
        obs = []
        for tr in bank.t:
            i, zr, zb = observe(rng, tr, lm, 10)
            zr[k % 10] += 20.0                                             # an outlier, as the gate tests inject them
            obs.append((i, zr, zb))
        kept = bank.step(np.full(2, 0.01), np.full(2, 0.05), obs)
        for b, (i, zr, zb) in enumerate(kept):
            assert set(i) <= set(obs[b][0].tolist())
    for rows in bank.ring().values():
        for idx, y, S, nis, rej in rows:
            assert ((nis <= g / fm.BAND) | (nis >= g * fm.BAND)).all()
            assert (rej == (nis > g)).all()
            rejected += int(rej.sum())
    assert rejected > 0 and rejected == sum(tr.rejections for tr in bank.t)
    assert bank.dropped > 0 or g == 25.0
    assert fm.ambiguous([g * 3.9], g) == 0 and fm.ambiguous([g * 4.0, g / 4.0], g) is None
    assert fm.ambiguous([1e9], math.inf) is None
