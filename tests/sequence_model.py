"""One dense model of ONE trajectory under the whole state-changing surface of a handle, for tests/sequence_cases.py.
(tests/sequence_bank_cases.py runs the same class over a BANK: see "A BANK" below; at B = 1 nothing differs.)

`SeqBank` is tests/fork_model.py's ForkBank (step, update, predict, predict_dense, grow, remove, window, copy_from) plus the
newer calls, each DELEGATED to the model the project already trusts -- no new mathematics:

    update_direct    direct_model.direct_update_joseph        update_linear    linear_model.linear_update_joseph
    predict_linear   motion_model.predict_linear              transform        transform_model.transform_dense
    join             join_model.join_dense (both modes)       set_state / set_state_diag, set_option: bookkeeping only
    localize1, localize_update1, run_localize_stream          localize_model.literal_step (the trajectory's own cfg)
    localize_detections                                       loc_det_world.model_window (frontend.associate_known, then
                                                              literal_step: Bank.window's arrangement for step_detections)
    hyp_adopt, hyp_resample_adopt                             literal_step per hypothesis; resample_model.plan / margin on the
                                                              model's own log-likelihoods, resample_model.split_dense

The methods carry EkfSlam's names and take ONE trajectory's arguments (b = 0), so that a sequence written once runs on the model
and on a filter (tests/sequence_cases.py's Driver).  The other handles a call reads (`join`, `copy_from`) are named by a key of
`sources`: key -> (mean, covariance, tag index).

`Traj.seen` follows each call's rule -- which landmarks are correlated with the rest: a dense-H row, a transform with a
covariance, a sequential join (what it appends) and predict_dense correlate everything they name; a direct fix of a
never-observed landmark and a transform without a covariance leave the exact zeros.  A localisation call makes every landmark it
names seen -- its pose cross-covariance becomes non-zero -- while the landmark's own block and mean do not move.

A BANK.  `SeqBank([(mean, diag), ...])` keeps one trajectory per start and a TARGET slot: `tr` is `t[target]`, and every
per-trajectory method above acts on the target (B = 1: slot 0, as ever).  The calls that take the whole bank at once carry one
entry per slot: bank_step, bank_stream, bank_detections, bank_localize, bank_localize_stream -- loops over Bank.step,
Bank.window and localize_model.literal_step, nothing else.  Two calls need a second slot of the SAME bank: `fork(src, dst)`
(ForkBank's, through copy_from) and `join_slot(src)`, join_model.join_dense with slot `src` as the source.

PRECISION.  `bank(..., dtype=np.longdouble)` runs the SAME functions in extended precision (x87: 64 bits of mantissa): the
models' code objects are re-bound to a namespace in which `np` is a proxy whose array constructors make `dtype` arrays
(`dtype=float` included) and whose `linalg.solve` / `linalg.inv` are a pivoted elimination in `dtype` (LAPACK has no extended
precision; the systems are at most 7 x 7).  Nothing of the models is restated.  Inputs -- measurements, noise constants,
Jacobians handed in -- are the same float64 values in both precisions; only the arithmetic differs."""
import dataclasses
import sys
import types

import numpy as np

from tests import direct_model as dm
from tests import join_model as jm
from tests import linear_model as lm
from tests import loc_det_world as ldw
from tests import localize_model as lcm
from tests import motion_model as mm
from tests import resample_model as rsm
from tests import transform_model as tm
from tests.fork_model import ForkBank
from tests.fuzz_model import Traj


class SeqBank(ForkBank):
    def __init__(self, mean0, diag0=None, sources=None, base=None):
        """(mean0, diag0): one trajectory; diag0 None: `mean0` is a list of (mean, diag) starts, one per slot of a bank."""
        starts = [(mean0, diag0)] if diag0 is not None else list(mean0)
        ForkBank.__init__(self, [(m, np.diag(np.asarray(d, dtype=float))) for m, d in starts], base)
        self.sources = dict(sources or {})
        self.target = 0

    @property
    def tr(self):
        return self.t[self.target]

    def state(self, b=None):
        """(mean, covariance, tag index) of the target trajectory (b given: of slot b)."""
        tr = self.tr if b is None else self.t[b]
        return tr.mean, tr.cov, dict(tr.tags)

    # -- bookkeeping ---------------------------------------------------------------------------------------------------------
    def set_state(self, mean, cov):
        old = self.tr
        self.t[self.target] = Traj(mean, cov, self.base)
        self.tr.cfg, self.tr.rejections = old.cfg, old.rejections
        d = np.diag(self.tr.cov)
        off = np.abs(self.tr.cov).sum(axis=0) - np.abs(d)
        self.tr.seen = (off[3::2] > 0) | (off[4::2] > 0)

    def set_state_diag(self, mean, diag):
        self.set_state(mean, np.diag(np.asarray(diag, dtype=float)))

    def set_tag_index(self, tags):
        self.tr.tags = {int(t): int(j) for t, j in tags.items()}

    def set_option(self, name, value):
        pass                                             # (the active bound changes no result)

    # -- the calls ForkBank has, for one trajectory (step1, run_stream, step_detections: a bank of ONE; a larger bank takes the
    #    bank_* calls below, which name every slot) ---------------------------------------------------------------------------
    def step1(self, lin, ang, idx, zr, zb):
        self.step([lin], [ang], [(list(idx), list(zr), list(zb))])

    def run_stream(self, lin, ang, idx, zr, zb):
        for k in range(len(lin)):
            self.step1(lin[k], ang[k], idx[k], zr[k], zb[k])

    def step_detections(self, lin, ang, win):
        self.window([lin], [ang], [win])

    def add_landmarks(self, xy):
        self.grow(xy, self.target)

    def remove_landmarks(self, lms):
        self.remove([int(l) for l in lms], self.target)

    def predict_dense1(self, F, Q):
        self.predict_dense(np.asarray(F, dtype=float), np.asarray(Q, dtype=float), self.target)

    def copy_in(self, key):
        """copy_from(the handle `key` names): this trajectory is the destination."""
        mean, cov, tags = self.sources[key]
        tr = self.tr
        tr.mean, tr.cov, tr.tags = np.array(mean, dtype=float), np.array(cov, dtype=float), dict(tags)
        tr.seen = np.ones(tr.n_lm, dtype=bool)

    # -- the newer calls, delegated ------------------------------------------------------------------------------------------
    def update_direct(self, targets, z, R):
        tr = self.tr
        tr.mean, tr.cov, _, _, applied = dm.direct_update_joseph(tr.mean, tr.cov, targets, z, R)
        assert applied

    def update_linear(self, landmarks, H, R, z):
        tr = self.tr
        tr.mean, tr.cov, _, _, applied = lm.linear_update_joseph(tr.mean, tr.cov, landmarks, H, R, z)
        assert applied
        tr.seen[np.asarray(landmarks, dtype=int)] = True

    def predict_linear(self, pose, F, Q):
        tr = self.tr
        tr.mean, tr.cov = mm.predict_linear(tr.mean, tr.cov, pose, F, Q)

    def transform(self, T, cov=None):
        tr = self.tr
        tr.mean, tr.cov = tm.transform_dense(tr.mean, tr.cov, T, cov)[:2]
        if cov is not None:
            tr.seen[:] = True

    def join(self, key, transform=None, cov=None):
        self._append(*self.sources[key], transform, cov)

    def join_slot(self, src, transform=None, cov=None):
        """join with slot `src` of this bank as the source (only read)."""
        assert src != self.target
        s = self.t[src]
        self._append(s.mean, s.cov, s.tags, transform, cov)

    def _append(self, mean, P, tags, transform, cov):
        tr = self.tr
        first, count = tr.n_lm, (len(mean) - 3) // 2
        tr.mean, tr.cov = jm.join_dense(tr.mean, tr.cov, mean, P, transform, cov, with_bound=False)[:2]
        tr.seen = np.concatenate([tr.seen, np.ones(count, dtype=bool)])
        for t, j in tags.items():                          # (a tag this map already holds: the appended twin carries none)
            tr.tags.setdefault(t, first + j)

    # -- localisation on a frozen map: localize_model.literal_step, one call per step -----------------------------------------
    def localize1(self, lin, ang, idx, zr, zb, predict=True):
        self._localize(self.tr, lin, ang, idx, zr, zb, predict)

    def _localize(self, tr, lin, ang, idx, zr, zb, predict):
        idx = [int(j) for j in idx]
        tr.mean, tr.cov = lcm.literal_step(tr.mean, tr.cov, lin, ang, idx, zr, zb, tr.cfg, predict=predict)
        tr.seen[np.asarray(idx, dtype=int)] = True

    def localize_update1(self, idx, zr, zb):
        self.localize1(0.0, 0.0, idx, zr, zb, predict=False)

    def run_localize_stream(self, lin, ang, idx, zr, zb):
        for k in range(len(lin)):
            self.localize1(lin[k], ang[k], idx[k], zr[k], zb[k])

    # -- localisation from raw detections: what the window matches, then one localisation step ---------------------------------
    def localize_detections(self, lin, ang, win, unmatched):
        self._localize_window(self.tr, lin, ang, win, unmatched)

    def _localize_window(self, tr, lin, ang, win, unmatched):
        (tr.mean, tr.cov), tags, un = ldw.model_window(tr.mean, tr.cov, tr.tags, win, lin, ang, cfg=tr.cfg)
        assert list(un) == list(unmatched), (un, unmatched)
        tr.seen[np.asarray(list(tags), dtype=int)] = True

    # -- a hypothesis bank on the target's map, stepped twice, one hypothesis adopted -------------------------------------------
    def hyp_adopt(self, motion, one, lists, k):
        """Step one with the shared list `one`, step two with one list per hypothesis: the slot ends as hypothesis k does."""
        self.localize1(*motion[0], *one)
        self.localize1(*motion[1], *lists[k])

    def hyp_resample_adopt(self, motion, one, two, pose0, cov0, u, s, z):
        """Hypothesis 0 reset to (pose0, cov0), step one for all three, the resampling plan from the model's own log-likelihoods
        (resample_model.plan; its margin keeps the plan from depending on rounding), the split, step two, slot 0 adopted."""
        tr = self.tr
        mean, cov = self._hyp_resampled(motion[0], one, pose0, cov0, u, s, z)
        tr.mean, tr.cov = lcm.literal_step(mean, cov, *motion[1], *two, tr.cfg)
        tr.seen[np.asarray(list(one[0]) + list(two[0]), dtype=int)] = True

    def _hyp_resampled(self, motion, one, pose0, cov0, u, s, z):
        """Slot 0 of the bank behind step one and the resampling: its ancestor's state, split."""
        tr = self.tr
        states, ll = [_reset(tr.mean, tr.cov, pose0, cov0), (tr.mean, tr.cov), (tr.mean, tr.cov)], np.zeros(3)
        for h in range(3):
            log = []
            states[h] = lcm.literal_step(*states[h], *motion, *one, tr.cfg, log=log)
            ll[h] = loglik(log)
        flags = np.zeros(3, dtype=np.uint32)
        anc, off, W = rsm.plan(ll, flags, u)
        assert anc[0] != 0 and off[0] == 0 and off[anc[0]] >= 2, (anc, off, ll)
        assert rsm.margin(ll, flags, u) >= 1e-6, (rsm.margin(ll, flags, u), ll)
        return rsm.split_dense(*states[anc[0]], s, np.asarray(z)[0])

    # -- the calls that take the whole bank: one entry per slot --------------------------------------------------------------
    def bank_step(self, lin, ang, obs):
        """step: lin, ang [B]; obs per slot (idx, zr, zb)."""
        self.step(list(lin), list(ang), [(list(i), list(r), list(z)) for i, r, z in obs])

    def bank_stream(self, lin, ang, idx, zr, zb, m):
        """run_stream: lin, ang [K, B]; idx, zr, zb [K, B, stride]; m [K, B] valid entries."""
        for k in range(len(lin)):
            self.bank_step(lin[k], ang[k], [(idx[k][b][:m[k][b]], zr[k][b][:m[k][b]], zb[k][b][:m[k][b]])
                                            for b in range(len(self.t))])

    def bank_detections(self, lin, ang, wins):
        self.window(list(lin), list(ang), list(wins))

    def bank_localize(self, lin, ang, obs, predict=True):
        for b, tr in enumerate(self.t):
            self._localize(tr, lin[b], ang[b], obs[b][0], obs[b][1], obs[b][2], predict)

    def bank_localize_stream(self, lin, ang, idx, zr, zb, m):
        for k in range(len(lin)):
            self.bank_localize(lin[k], ang[k], [(idx[k][b][:m[k][b]], zr[k][b][:m[k][b]], zb[k][b][:m[k][b]])
                                                for b in range(len(self.t))])

    def bank_localize_detections(self, lin, ang, wins, unmatched):
        for b, tr in enumerate(self.t):
            self._localize_window(tr, lin[b], ang[b], wins[b], unmatched[b])


def _reset(mean, cov, pose, block):
    """reset_pose on a dense state (hypotheses_model.reset_state): the pose and its block replaced, the cross terms dropped."""
    mean, cov = np.array(mean), np.array(cov)
    mean[:3] = pose
    cov[:3, :], cov[:, :3] = 0.0, 0.0
    cov[:3, :3] = block
    return mean, cov


def loglik(log):
    """The sum a hypothesis accumulates, from literal_step's records (hypotheses_model.loglik_of; det S of a 2 x 2 written out:
    LAPACK has no extended precision)."""
    return sum(-0.5 * (nis + np.log(S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) + 2.0 * np.log(2.0 * np.pi)) for _, _, S, nis, _ in log)


# ---- the same code in another precision --------------------------------------------------------------------------------------
_REBOUND = ("oracle.ekf_oracle", "tests.gated_oracle","tests.fuzz_model", "tests.fork_model", "tests.direct_model",
            "tests.linear_model", "tests.localize_model", "tests.motion_model", "tests.transform_model", "tests.join_model",
            "tests.loc_det_world", "tests.resample_model", __name__)
_CLASSES = ("Traj", "Bank", "ForkBank", "SeqBank")


def _elimination(dt):
    def solve(A, B):
        A, B = np.array(A, dtype=dt), np.array(B, dtype=dt)
        n = len(A)
        X = B.reshape(n, -1).copy()
        for k in range(n):
            p = k + int(np.argmax(np.abs(A[k:, k])))
            if p != k:
                A[[k, p]], X[[k, p]] = A[[p, k]], X[[p, k]]
            for i in range(k + 1, n):
                f = A[i, k] / A[k, k]
                A[i, k:] -= f * A[k, k:]
                X[i] -= f * X[k]
        for k in range(n - 1, -1, -1):
            X[k] = (X[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
        return X.reshape(B.shape)

    return types.SimpleNamespace(solve=solve, inv=lambda A: solve(A, np.eye(len(A), dtype=dt)), norm=np.linalg.norm)


class _Numpy:
    """numpy, but floating-point arrays are made in `dt`."""

    def __init__(self, dt):
        self._dt, self.linalg = dt, _elimination(dt)

    def __getattr__(self, name):
        return getattr(np, name)

    def _d(self, dtype):
        return self._dt if dtype is None or dtype is float else dtype

    def zeros(self, shape, dtype=None):
        return np.zeros(shape, self._d(dtype))

    def ones(self, shape, dtype=None):
        return np.ones(shape, self._d(dtype))

    def empty(self, shape, dtype=None):
        return np.empty(shape, self._d(dtype))

    def full(self, shape, value, dtype=None):
        return np.full(shape, value, self._d(dtype))

    def eye(self, N, M=None, k=0, dtype=None):
        return np.eye(N, M, k, self._d(dtype))

    def _floating(self, a):
        return a.astype(self._dt) if a.dtype.kind == "f" and a.dtype != self._dt else a

    def array(self, obj, dtype=None, **kw):
        return self._floating(np.array(obj, dtype=None if dtype is float else dtype, **kw))

    def asarray(self, obj, dtype=None, **kw):
        return self._floating(np.asarray(obj, dtype=None if dtype is float else dtype, **kw))


def _rebind(name, npx, memo):
    """The module `name` as a namespace whose functions and model classes see `npx` for numpy and one another's re-bound
    versions: the same code objects, other globals."""
    if name in memo:
        return memo[name]
    mod = sys.modules[name]
    ns = types.SimpleNamespace()
    g = ns.__dict__
    g.update(vars(mod))
    memo[name] = ns

    def fn(v):
        new = types.FunctionType(v.__code__, g, v.__name__, v.__defaults__, v.__closure__)
        new.__kwdefaults__ = v.__kwdefaults__
        return new

    for key, v in list(g.items()):
        if v is np:
            g[key] = npx
        elif isinstance(v, types.ModuleType) and v.__name__ in _REBOUND:
            g[key] = _rebind(v.__name__, npx, memo)
        elif isinstance(v, types.FunctionType) and v.__module__ in _REBOUND:
            g[key] = fn(v) if v.__module__ == name else getattr(_rebind(v.__module__, npx, memo), v.__name__)
        elif isinstance(v, type) and v.__name__ in _CLASSES and v.__module__ in _REBOUND and not dataclasses.is_dataclass(v):
            if v.__module__ != name:
                g[key] = getattr(_rebind(v.__module__, npx, memo), v.__name__)
                continue
            bases = tuple(getattr(_rebind(b.__module__, npx, memo), b.__name__) if b.__name__ in _CLASSES else b
                          for b in v.__bases__)
            body = {k: (fn(a) if isinstance(a, types.FunctionType) else
                        property(fn(a.fget)) if isinstance(a, property) else a)
                    for k, a in vars(v).items() if k not in ("__dict__", "__weakref__")}
            g[key] = type(v.__name__, bases, body)
    return ns


_BANKS = {}


def bank(mean0, diag0, sources=None, dtype=np.float64):
    """A SeqBank in `dtype`: float64 is the class above as it stands, anything else the re-bound copy.  (diag0 None: `mean0`
    is a list of starts, one per slot.)"""
    dt = np.dtype(dtype)
    if dt == np.float64:
        return SeqBank(mean0, diag0, sources)
    if dt not in _BANKS:
        _BANKS[dt] = _rebind(__name__, _Numpy(dt), {}).SeqBank
    return _BANKS[dt](mean0, diag0, sources)
