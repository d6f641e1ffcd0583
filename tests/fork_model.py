"""tests/fuzz_model.py's Bank with device-side forks (EkfSlam.fork / copy_from), and one seeded interleaving of
step / grow / remove / fork that tests/test_fork_cpu.py runs on the model alone and tests/test_gpu_fork.py on the model and a
filter side by side.

A copy moves the STATE of a trajectory -- mean, covariance, which landmarks have been touched, the tag table -- and leaves
the properties of the SLOT: its noise row, its rejection count; it writes no log row.  The invariants `drive` asserts:
  * right after a fork every destination's state is the source's, bit for bit;
  * TWINS STAY TWINS: two trajectories whose model states are bit-identical and whose noise rows are equal are bit-identical
    on the filter too, whatever ran in between (the model gives twins the same observations);
  * slot properties are untouched by a fork: noise rows, gate counts, the number of logged steps;
  * every trajectory equals the model within `tol`."""
import copy

import numpy as np

from oracle import ekf_oracle as orc
from tests.fuzz_model import Bank
from tests.gpu_support import same as same_state


class ForkBank(Bank):
    def copy_from(self, other, src=0, dst=0):
        src, dst = np.atleast_1d(src).astype(int), np.atleast_1d(dst).astype(int)
        if src.shape != dst.shape:
            raise ValueError("copy_from: src and dst must have the same length")
        if len(set(dst.tolist())) != len(dst):
            raise ValueError("copy_from: a destination named twice")
        if other is self and set(src.tolist()) & set(dst.tolist()):
            raise ValueError("copy_from: a trajectory both read and written")
        for s, d in zip(src, dst):
            a, b = other.t[s], self.t[d]
            b.mean, b.cov, b.seen, b.tags = a.mean.copy(), a.cov.copy(), a.seen.copy(), dict(a.tags)

    def fork(self, src=0, dst=None):
        if dst is None:
            dst = [b for b in range(len(self.t)) if b != src]
        dst = np.atleast_1d(dst).astype(int)
        self.copy_from(self, np.full(dst.shape, int(src)), dst)


def slot_properties(model):
    return ([dataclass_pair(tr.cfg) for tr in model.t], [tr.rejections for tr in model.t], model.log_steps)


def dataclass_pair(cfg):
    return (cfg.motion_sigma, cfg.meas_sigma)


def observations(model, rng, m):
    """m landmarks every trajectory has, seen from each trajectory's own model pose, with ONE noise draw for the whole bank
    (twins get identical observations)."""
    n_lo = min(tr.n_lm for tr in model.t)
    idx = rng.choice(n_lo, size=min(m, n_lo), replace=False)
    nr, nb = rng.normal(0, 0.01, len(idx)), rng.normal(0, 0.005, len(idx))
    obs = []
    for tr in model.t:
        d = tr.mean[3:].reshape(-1, 2)[idx] - tr.mean[0:2]
        zr = np.hypot(d[:, 0], d[:, 1]) + nr
        zb = np.arctan2(d[:, 1], d[:, 0]) - tr.mean[2] + nb
        obs.append((idx.tolist(), zr.tolist(), zb.tolist()))
    return obs


def start_states(N, B, seed):
    out = []
    for b in range(B):
        mean0, diag0 = orc.synthetic_stream(N, 1, 4, seed + b)[:2]
        out.append((mean0, np.diag(np.minimum(diag0, 4.0))))
    return out


def drive(model, seed, ops, n_cap, f=None, tol=None):
    """`ops` seeded operations on `model` (a ForkBank) and, if given, on the filter `f` holding the same states.  n_cap: the
    landmark capacity (grow stops there).  Returns how many of each operation ran."""
    rng = np.random.default_rng(seed)
    B = len(model.t)
    ran = {"step": 0, "grow": 0, "remove": 0, "fork": 0}

    def check_twins():
        if f is None:
            return
        got = [f.state(b) for b in range(B)]
        for a in range(B):
            assert orc.rel_fro(got[a][0], model.t[a].mean) < tol and orc.rel_fro(got[a][1], model.t[a].cov) < tol, a
            for b in range(a + 1, B):
                twins = (same_state((model.t[a].mean, model.t[a].cov), (model.t[b].mean, model.t[b].cov))
                         and dataclass_pair(model.t[a].cfg) == dataclass_pair(model.t[b].cfg))
                if twins:
                    assert same_state(got[a], got[b]), (a, b)

    for _ in range(ops):
        op = rng.choice(["step", "step", "step", "grow", "remove", "fork"])
        if op == "step":
            lin, ang = np.full(B, 0.004), np.full(B, float(rng.choice([0.02, 0.005])))
            kept = model.step(lin, ang, observations(model, rng, int(rng.integers(0, 6))))
            if f is not None:
                f.step(lin, ang, [k[0] for k in kept], [k[1] for k in kept], [k[2] for k in kept])
        elif op == "grow":
            b = int(rng.integers(B))
            if model.t[b].n_lm + 2 > n_cap:
                continue
            xy = rng.uniform(-1.0, 1.0, (int(rng.integers(1, 3)), 2))
            model.grow(xy, b)
            if f is not None:
                f.add_landmarks(xy, b)
        elif op == "remove":
            b = int(rng.integers(B))
            if model.t[b].n_lm <= 4:
                continue
            lm = [int(rng.integers(model.t[b].n_lm))]
            model.remove(lm, b)
            if f is not None:
                f.remove_landmarks(lm, b)
        else:
            src = int(rng.integers(B))
            others = [b for b in range(B) if b != src]
            dst = sorted(rng.choice(others, size=int(rng.integers(1, B)), replace=False).tolist())
            props = copy.deepcopy(slot_properties(model))
            model.fork(src, dst)
            assert slot_properties(model) == props
            for d in dst:
                assert same_state((model.t[d].mean, model.t[d].cov), (model.t[src].mean, model.t[src].cov))
                assert model.t[d].tags == model.t[src].tags and np.array_equal(model.t[d].seen, model.t[src].seen)
            if f is not None:
                noise, counts, logged = f.noise(), f.gate_counts(), f.innovations().steps.shape[0]
                want = f.state(src)
                f.fork(src, dst)
                for d in dst:
                    assert same_state(f.state(d), want) and f.size(d) == f.size(src) and f.flags(d) == f.flags(src)
                assert np.array_equal(f.noise()[0], noise[0]) and np.array_equal(f.noise()[1], noise[1])
                assert np.array_equal(f.gate_counts(), counts) and f.innovations().steps.shape[0] == logged
        ran[op] += 1
        check_twins()
    return ran
