"""Randomised mixed-API runs over the whole filter surface against the oracle model of tests/fuzz_model.py.

tests/test_gpu_fuzz.py mixes steps, streams, flushes, dense products, growth and option changes.  Here the same kinds of
sequence also carry the newer calls: per-trajectory noise (`set_noise`, changed with ranks pending and between the two
pieces of a stream), the NIS gate (on, off, by threshold or confidence, with injected outliers), the innovation log
(`log_innovations`, rings that wrap, re-enabled), landmark removal (per trajectory and whole bank, with ranks pending, across
the column-panel boundary, stale streams), `step_detections` (device association and the host fallback beyond the device
limits, with the noise table on) and `marginals`.  At random points and at the end every checked trajectory's state is
compared block by block with the model (tests/parity_blocks.py), marginals with the model's blocks and with a download
taken right after, the log and the gate counts with the model's records, sizes and tags with the model's map.

A shadow handle gets the same calls minus those documented as result-neutral (no marginals / innovations / gate_counts /
noise(), never the log; the gate off where the main handle has a threshold no update reaches; no noise table where the main
handle's rows equal the config) and must stay bit-identical: states, flags and the scheduling counters.

Every case names the path it ran; the last test asserts that the module reached each promise it makes."""
import math

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import fuzz_model as fm
from tests import parity_blocks as pb
from tests.conftest import path_ran
from tests.gated_oracle import check_gated_entries
from tests.gpu_support import raw00, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-8              # (long random sequences from 1e4 initial variances: tests/test_gpu_fuzz.py's TIGHT)
MARG_TOL = 1e-10        # marginals against the blocks of a download taken right after them
INERT = 1e300
G = 25.0
CONF = 0.99
BASE = orc.EkfConfig()

# name: (seed, N, B, small_state, ops, spare landmarks, distinct tag ids, path)
CASES = {
    "small_n20x3": (1, 20, 3, 1, 40, 18, 8, "small"),
    "general_n30x2": (2, 30, 2, 0, 40, 50, 40, "general"),
    "small_bank_n50x128": (3, 50, 128, 1, 22, 14, 8, "small"),
    "chained_n150x3": (4, 150, 3, 0, 36, 50, 40, "chained"),
    "bound_n400x2": (5, 400, 2, 0, 30, 50, 40, "active_bound"),
    "panels_n2100x1": (6, 2100, 1, 0, 16, 50, 40, "panels"),
    # the smallest bank plan_pass sends to the row-slab pass: streaming (B 8 n^2 > 192 MB) with B x (128-row slabs) of at
    # least 2.35 per CU (256 CUs) -- 208 x N = 190 (n = 383, three slabs)
    "rowslab_n190x208": (7, 190, 208, 0, 14, 6, 6, "rowslab"),
}
PROMISES = {"removal_pending": 0, "marginals_pending": 0, "rejections": 0, "wraps": 0, "detections_distinct_noise": 0,
            "fallbacks": 0, "stale_refused": 0, "whole_bank_removal": 0}
RAN = set()


def pending(sd, f, bank, b):
    """Rank terms pending in trajectory b: the stored P_base[0, 0] is not yet the model's."""
    want = bank.t[b].cov[0, 0]
    return abs(raw00(sd, f, b) - want) > 1e-6 * abs(want)


def sched(sd, f):
    lib = sd.load_library()
    return f.cadence_counters(), lib.ekf_debug_chained(f._h), lib.ekf_debug_small_launches(f._h)


def blocks(P):
    nl = (P.shape[0] - 3) // 2
    r = 3 + 2 * np.arange(nl)
    return P[:3, :3], np.stack([np.stack([P[r, r], P[r, r + 1]], -1), np.stack([P[r + 1, r], P[r + 1, r + 1]], -1)], -2)


def stacked_err(got, want):
    return orc.rel_fro(np.concatenate([got[0].ravel(), got[1].ravel()]), np.concatenate([want[0].ravel(), want[1].ravel()]))


def observe(rng, tr, m, outliers):
    """m distinct landmarks measured from the model's own estimate + noise; with `outliers` one of them at range + 20 m."""
    m = min(m, tr.n_lm)
    idx = rng.choice(tr.n_lm, size=m, replace=False).astype(np.int32)
    d = np.stack([tr.mean[3 + 2 * idx], tr.mean[4 + 2 * idx]], 1) - tr.mean[0:2]
    zr = np.maximum(np.hypot(d[:, 0], d[:, 1]) + rng.normal(0, 0.02, m), 0.05)
    zb = np.arctan2(d[:, 1], d[:, 0]) - tr.mean[2] + rng.normal(0, 0.02, m)
    if outliers and m and rng.random() < 0.5:
        zr[int(rng.integers(0, m))] += 20.0
    return idx, zr, zb


def noise_rows(rng, B):
    return rng.uniform(0.03, 0.3, B), rng.uniform(0.2, 1.5, B)


def run_case(sd, name):
    seed, N, B, small, n_ops, spare, n_ids, path = CASES[name]
    rng = np.random.default_rng(7000 + seed)
    cap_lm = N + spare
    n_max = 3 + 2 * cap_lm
    states = []
    dense = path == "rowslab"                                   # (a dense start: every index active, three slabs)
    for b in range(B):
        truth = np.stack([rng.uniform(-1.0, 1.0, N), rng.uniform(-0.8, 1.2, N)], 1)
        mean = np.concatenate([[0.0, 0.0, 0.0], (truth + rng.normal(0, 0.05, truth.shape)).ravel()])
        diag = np.concatenate([[0.1, 0.1, 0.1], np.full(2 * N, 1.0e4 if not dense else 0.05)])
        states.append((mean, np.diag(diag)))
    bank = fm.Bank(states)
    ids = [int(i) for i in rng.permutation(1000)[:n_ids]]
    new_xz = {i: (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.4, 1.1))) for i in ids}
    checked = sorted({0, B - 1, *[int(x) for x in rng.integers(0, B, 2)]})
    ops = []
    seen = {"rs": False, "bound": set(), "panel_removal": False, "marginals": False, "fallback": False}
    lib = sd.load_library()
    f, s = sd.EkfSlam(n_max, batch=B), sd.EkfSlam(n_max, batch=B)
    handles = (f, s)
    gate_main = None                                            # what the main handle's gate is set to
    stream_up = False

    def both(fn):
        return [fn(h) for h in handles]

    def check(b, what):
        tr = bank.t[b]
        (mu, P), (smu, sP) = f.state(b), s.state(b)
        assert f.flags(b) == 0 and s.flags(b) == 0, what
        assert np.array_equal(P, P.T), f"{what}: covariance of trajectory {b} not exactly symmetric"
        assert np.array_equal(mu, smu) and np.array_equal(P, sP), f"{what}: trajectory {b} differs from the shadow"
        assert sched(sd, f) == sched(sd, s), f"{what}: scheduling differs from the shadow"
        assert f.size(b) == len(tr.mean) == s.size(b)
        assert {t: j for t, j in f.tag_index(b).items() if t >= 0} == tr.tags, f"{what}: tag index of trajectory {b}"
        assert s.tag_index(b) == f.tag_index(b)
        r = orc.rel_fro(P, tr.cov)
        assert r < TOL, f"{what}: covariance of trajectory {b}: rel Frobenius {r:.3e}"
        assert orc.rel_fro(mu, tr.mean) < TOL
        obs = tr.observed()
        if len(obs):
            pb.assert_filter_close(mu, P, tr.mean, tr.cov, obs, tol=TOL, what=f"{what}: trajectory {b}: ")
        if seen["rs"] is False and "k_flush_rs" in f.last_pass():
            seen["rs"] = True

    def check_log(what):
        if not bank.log_cap:
            return
        innov = f.innovations()
        ring = bank.ring()
        assert innov.steps.tolist() == sorted(ring), f"{what}: logged steps {innov.steps.tolist()} != {sorted(ring)}"
        if bank.log_steps > bank.log_cap:
            PROMISES["wraps"] += 1
        for k, step in enumerate(sorted(ring)):
            for b in checked:
                idx, ys, Ss, nis, rej = ring[step][b]
                check_gated_entries(innov, k, b, idx, ys, Ss, nis, rej)

    def check_gate(what):
        got = f.gate_counts()
        want = [tr.rejections for tr in bank.t]
        assert got.tolist() == want, f"{what}: gate counts {got.tolist()} != {want}"

    def outliers():
        return gate_main is not None and math.isfinite(bank.gate) and bank.gate < 1e3

    try:
        full = dense | (rng.random(B) < 0.5)
        for h in handles:
            h.set_option("small_state", small)
            for b, (mean, cov) in enumerate(states):
                if full[b]:
                    h.set_state(mean, cov, b)
                else:
                    h.set_state_diag(mean, np.diag(cov), b)
        f.log_innovations(int(rng.choice([3, 5, 16])))
        bank.log_innovations(f._innov_cap)
        force = {n_ops // 3: ("active_bound", 0), 2 * n_ops // 3: ("active_bound", 1)} if path == "active_bound" else {}
        force_op = {n_ops // 2: "remove", n_ops // 2 + 1: "marginals"} if path == "panels" else {}
        for it in range(n_ops):
            op = str(rng.choice(["step", "step", "predict", "update", "step_state", "grow", "stream", "stream", "flush", "dense",
                                 "option", "noise", "noise", "gate", "log", "remove", "remove", "window", "window",
                                 "marginals", "download"]))
            if it in force:
                op = "option"
            op = force_op.get(it, op)
            lin = rng.uniform(0.002, 0.02, B)
            ang = np.where(rng.random(B) < 0.3, rng.uniform(-0.008, 0.008, B), rng.uniform(-0.3, 0.3, B))
            mhi = 4 if N > 1000 else 10
            if op in ("step", "step_state", "update"):
                m = int(rng.integers(0 if op != "update" else 1, (mhi if op != "update" else 20) + 1))
                obs = [observe(rng, tr, m, outliers()) for tr in bank.t]
                if op == "update":
                    kept = bank.update(obs)
                    both(lambda h: h.update(*[[o[i] for o in kept] for i in range(3)]))
                else:
                    kept = bank.step(lin, ang, obs)
                    args = (lin, ang) + tuple([o[i] for o in kept] for i in range(3))
                    if op == "step":
                        both(lambda h: h.step(*args))
                    else:
                        b = int(rng.integers(0, B))
                        (mu, P), (smu, sP) = both(lambda h: h.step_state(*args, b=b))
                        assert np.array_equal(mu, smu) and np.array_equal(P, sP)
                        assert orc.rel_fro(P, bank.t[b].cov) < TOL and orc.rel_fro(mu, bank.t[b].mean) < TOL
                op += f"(m={m})"
            elif op == "predict":
                bank.predict(lin, ang)
                both(lambda h: h.predict(lin, ang))
            elif op == "grow":
                b = int(rng.integers(0, B))
                k = int(rng.integers(1, 4))
                if bank.t[b].n_lm + k + n_ids - len(bank.t[b].tags) <= cap_lm:     # (room left for every tag id)
                    xy = rng.uniform(-1.0, 1.0, (k, 2))
                    bank.grow(xy, b)
                    both(lambda h: h.add_landmarks(xy, b))
                    op += f"({b},{k})"
            elif op == "stream":
                steps = int(rng.integers(1, 5 if N > 1000 else 12))
                mcap = int(rng.choice([1, 2, 4, 8] if N <= 1000 else [1, 2, 4]))
                cut = int(rng.integers(0, steps + 1))
                switch = noise_rows(rng, B) if rng.random() < 0.35 else None
                idx = np.zeros((steps, B, mcap), dtype=np.int32)
                zr, zb = np.zeros((steps, B, mcap)), np.zeros((steps, B, mcap))
                ms = np.zeros((steps, B), dtype=np.int32)
                lins, angs = rng.uniform(0.002, 0.02, (steps, B)), rng.uniform(-0.2, 0.2, (steps, B))
                angs[rng.random((steps, B)) < 0.2] = 0.004
                for k in range(steps):
                    if k == cut and switch is not None:
                        bank.set_noise(*switch)
                    obs = [observe(rng, tr, int(rng.integers(0, mcap + 1)), outliers()) for tr in bank.t]
                    kept = bank.step(lins[k], angs[k], obs)
                    for b, o in enumerate(kept):
                        ms[k, b] = len(o[0])
                        idx[k, b, :ms[k, b]], zr[k, b, :ms[k, b]], zb[k, b, :ms[k, b]] = o
                if switch is not None and cut == steps:         # (a switch behind the last step: for the calls after it)
                    bank.set_noise(*switch)
                both(lambda h: h.stream_upload(lins, angs, idx, zr, zb, ms))
                stream_up = True
                both(lambda h: h.stream_run(0, cut))
                if switch is not None:                           # (between the two pieces: ranks of the first still pending)
                    both(lambda h: h.set_noise(*switch))
                if rng.random() < 0.3 and cut:
                    b = int(rng.integers(0, B))
                    both(lambda h: h.mean(b))
                both(lambda h: h.stream_run(cut, steps - cut))
                op += f"({steps},{cut}{',noise' if switch is not None else ''})"
            elif op == "flush":
                both(lambda h: h.flush())
            elif op == "dense" and len(bank.t[0].mean) <= 810:
                b = int(rng.integers(0, B))
                n = len(bank.t[b].mean)
                F = np.eye(n) + rng.normal(size=(n, n)) * (0.05 / np.sqrt(n))
                A = rng.normal(size=(n, 3)) * 0.02
                Q = A @ A.T + np.diag(rng.uniform(1e-4, 1e-3, n))
                bank.predict_dense(F, Q, b)
                both(lambda h: h.predict_dense(F, Q, b))
            elif op == "option":
                opts = [("flush_every", int(rng.integers(0, 6))), ("fused_cadence", int(rng.integers(0, 2))),
                        ("fused_step", int(rng.integers(0, 2))), ("lookahead", int(rng.integers(0, 2))),
                        ("rank_limit", int(rng.choice([16, 32, 48, 80]))), ("active_bound", int(rng.integers(0, 2))),
                        ("chain", int(rng.integers(0, 2))), ("run_end_flush", int(rng.integers(0, 2)))]
                if path != "rowslab":
                    opts += [("pass_kernel", int(rng.choice([-1, 0, 2]))), ("pass_streaming", int(rng.choice([-1, 0, 1])))]
                name_, value = force.get(it) or opts[int(rng.integers(0, len(opts)))]
                both(lambda h: h.set_option(name_, value))
                if name_ == "active_bound":
                    seen["bound"].add(value)
                op = f"{name_}={value}"
            elif op == "noise":
                kind = str(rng.choice(["scalar", "rows", "one_none", "reset", "equal"]))
                ms, qs = noise_rows(rng, B)
                if kind == "scalar":
                    args = (float(ms[0]), float(qs[0]))
                elif kind == "rows":
                    args = (ms, qs)
                elif kind == "one_none":
                    args = (ms, None) if rng.random() < 0.5 else (None, qs)
                else:
                    args = (None, None)
                bank.set_noise(*args)
                if kind == "equal":                              # rows equal to the config: the shadow has no table
                    f.set_noise(BASE.motion_sigma, BASE.meas_sigma)
                    s.set_noise()
                else:
                    both(lambda h: h.set_noise(*args))
                got = f.noise()
                want = bank.noise()
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                op += f"({kind})"
            elif op == "gate":
                kind = str(rng.choice(["off", "threshold", "confidence", "inert"]))
                if kind == "off":
                    gate_main, g = None, None
                    both(lambda h: h.set_nis_gate())
                elif kind == "threshold":
                    gate_main, g = G, G
                    both(lambda h: h.set_nis_gate(G))
                elif kind == "confidence":
                    gate_main, g = CONF, sd.EkfSlam.nis_gate_threshold(confidence=CONF)
                    both(lambda h: h.set_nis_gate(confidence=CONF))
                else:
                    gate_main, g = INERT, INERT
                    f.set_nis_gate(INERT)
                    s.set_nis_gate()
                bank.set_nis_gate(g)
                op += f"({kind})"
            elif op == "log":
                cap = int(rng.choice([0, 2, 3, 4, 8]))
                f.log_innovations(cap)
                bank.log_innovations(cap)
                op += f"({cap})"
            elif op == "remove":
                whole = rng.random() < 0.35 and it not in force_op
                b = None if whole else int(rng.integers(0, B))
                nl = min(tr.n_lm for tr in bank.t) if whole else bank.t[b].n_lm
                kind = "boundary" if it in force_op else str(rng.choice(["none", "one", "boundary", "run"]))
                if kind == "boundary":                           # column panels: state index 4096 (landmark 2046)
                    mid = 2046 if n_max > 4096 else nl // 2
                    lms = [l for l in range(mid - 2, mid + 3) if 0 <= l < nl]
                    if n_max > 4096:
                        seen["panel_removal"] = True
                elif kind == "run":
                    a = int(rng.integers(0, max(1, nl - 12)))
                    lms = list(range(a, min(nl, a + int(rng.integers(5, 13)))))
                elif kind == "one":
                    lms = [int(rng.integers(0, nl))]
                else:
                    lms = []
                if nl - len(lms) < 12:
                    lms = []
                b0 = 0 if whole else b
                if lms and pending(sd, f, bank, b0):
                    PROMISES["removal_pending"] += 1
                want = bank.remove(lms, b)
                got = both(lambda h: h.remove_landmarks(lms, b))
                assert np.array_equal(got[0], got[1])
                if b is not None or len({tr.n_lm for tr in bank.t}) == 1:
                    assert np.array_equal(got[0][:len(want)], want)
                PROMISES["whole_bank_removal"] += int(whole and bool(lms))
                if stream_up and lms:                            # the stream uploaded before is stale now
                    for h in handles:
                        with pytest.raises(sd.EkfError, match="upload the stream again"):
                            h.stream_run(0, 1)
                    PROMISES["stale_refused"] += 1
                    stream_up = False
                    check(0 if whole else b, f"op {it}: stale stream_run refused")
                op += f"({'all' if whole else b},{kind},{len(lms)})"
            elif op == "window":
                wins = []
                big = rng.random() < 0.3
                for tr in bank.t:
                    room = cap_lm - tr.n_lm
                    if big and room >= 34 and n_ids >= 34:       # more than 32 distinct tags
                        w = fm.window_of(rng, tr, ids[:34], new_xz, 1)
                    elif big:                                    # more than 256 detections
                        pick = [i for i in ids if i in tr.tags][:6] or ids[:min(4, room)]
                        w = fm.window_of(rng, tr, pick, new_xz, 1)
                        w = [(0.01 * fr, w[0][1]) for fr in range(257 // max(1, len(w[0][1])) + 1)] if w[0][1] else w
                    else:
                        k = int(rng.integers(1, min(10, n_ids) + 1))
                        pick = [int(i) for i in rng.choice(ids, size=k, replace=False)]
                        w = fm.window_of(rng, tr, pick, new_xz, int(rng.integers(1, 4)))
                    wins.append(w)
                before = f.assoc_fallbacks()
                kept, orders = bank.window(lin, ang, wins)
                assert all(tr.n_lm <= cap_lm for tr in bank.t)
                both(lambda h: h.step_detections(lin, ang, kept))
                if f.assoc_fallbacks() > before:
                    seen["fallback"] = True
                    PROMISES["fallbacks"] += 1
                elif seen["fallback"]:
                    raise AssertionError("a window after a host fallback went to the device association")
                if len(set(bank.noise()[0])) > 1 or len(set(bank.noise()[1])) > 1:
                    PROMISES["detections_distinct_noise"] += 1
                for b in checked:
                    order, tags = orders[b]
                    tp = f.tags_positions(b)
                    assert list(tp.keys()) == order, f"op {it}: tags_positions of trajectory {b}"
                    assert [tp[j][3] for j in order] == [tags[j][3] for j in order]
                op += f"({'big' if big else 'small'}, fallback={seen['fallback']})"
            elif op == "marginals":
                whole = rng.random() < 0.4
                bs = checked if whole else [int(rng.choice(checked))]
                pend = any(pending(sd, f, bank, b) for b in bs)
                PROMISES["marginals_pending"] += int(pend)
                if whole:
                    pose, lms, counts = f.marginals()
                    got = {b: (pose[b], lms[b, :counts[b]]) for b in bs}
                    assert all(counts[t] == bank.t[t].n_lm for t in range(B))
                else:
                    got = {bs[0]: f.marginals(bs[0])}
                for b in bs:
                    tr = bank.t[b]
                    assert len(got[b][1]) == tr.n_lm
                    if len(tr.observed()):
                        pb.assert_marginals_close(*got[b], tr.cov, tr.observed(), tol=TOL, what=f"op {it}: trajectory {b}: ")
                for b in bs:                                     # the blocks of a download taken right after
                    ref = blocks(f.state(b)[1])
                    s.state(b)
                    assert stacked_err(got[b], ref) < MARG_TOL, (b, stacked_err(got[b], ref))
                    again = f.marginals(b)                       # nothing pending now: the same bits
                    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
                seen["marginals"] = True
                op += f"({'all' if whole else bs[0]}, pending={pend})"
            ops.append(op)
            if op == "download" or rng.random() < 0.25:
                check(int(rng.choice(checked)), f"op {it}")
                check_log(f"op {it}")
                check_gate(f"op {it}")
        for b in checked:
            check(b, "end")
        check_log("end")
        check_gate("end")
        PROMISES["rejections"] += int(f.gate_counts().sum() > 0) + sum(
            int(r[4].sum()) for rows in bank.ring().values() for r in rows)
        # the path this case names
        if path == "small":
            assert path_ran(f, "default_path") and lib.ekf_debug_small_launches(f._h) > 0
        elif path == "general":
            assert path_ran(f, "general_kernels")
        elif path == "chained":
            assert lib.ekf_debug_chained(f._h) > 0
        elif path == "active_bound":
            assert seen["bound"] == {0, 1}
        elif path == "panels":
            assert f.n_max > 4096 and seen["panel_removal"] and seen["marginals"]
        elif path == "rowslab":
            assert seen["rs"], f"the row-slab pass never ran (last: {f.last_pass()!r})"
        print(f"{name}: {len(ops)} ops, {bank.dropped} observations dropped by the margin filter, checked {checked}, "
              f"last pass {f.last_pass()!r}")
    except AssertionError as e:
        raise AssertionError(f"{name}: {e}\nlast ops: {ops[-8:]}") from e
    finally:
        f.close()
        s.close()
    RAN.add(name)


@pytest.mark.parametrize("name", list(CASES))
def test_random_sequences_over_the_whole_surface(sd, name):
    run_case(sd, name)


def test_module_reached_every_promise():
    """Not vacuous: at least one removal and one marginals call with ranks pending, rejections, a wrapped ring, windows with
    distinct noise rows and beyond the device limits, a stale stream refused, a whole-bank removal."""
    if RAN != set(CASES):
        pytest.skip("needs every case of the module in the same run")
    missing = [k for k, v in PROMISES.items() if v == 0]
    assert not missing, f"never reached: {missing} ({PROMISES})"
