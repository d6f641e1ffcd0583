"""The case table of the geometry tests: scripts -- a start (mean, covariance, config) and twelve steps of
(lin, ang, [(landmark, range, bearing), ...]) -- grouped into banks of at most 16 slots that share a config, so that one handle
runs many.  NumPy, the oracle and tests/streams.py only; a plain module the CPU and GPU tests import.

Every script has N = 12 landmarks (n = 27) and at most four observations a step.  A stream script applies 47 or 48 landmark
updates, so that the fused cadence's 40 slots end inside it: with four observations in every step, step 10 opens the second
cadence (its prediction is the head of a cadence); with three in step 3 (`cut=True`), step 10 is cut by the boundary -- one
landmark closes the first cadence, three open the second without a second prediction.  The landmarks enter in a fixed order
(ORDER): first observations fall on step 0 (all four positions), on steps inside the first cadence, and on steps 10 and 11,
position 0 included; everything else re-observes.  In a diagonal start the landmarks observed exactly once (ONCE) begin at
variance 1e4, the others at 0.05^2: a second look at a landmark whose 1e4 has just collapsed to ~0.5 reads a block that float64
holds to 1e4 eps = 2e-12 only, which is the reference's own error and would cost the 1e-12 condition on S, not a device's.

A script is built against the float64 oracle as it runs: a landmark's mean is set when it is first observed -- to the range
and world direction the case asks for, seen from the oracle's pose of that moment (nothing before its first observation reads a
landmark's mean, so this only fixes the start) -- and every measurement is the oracle's own prediction plus a residual: range
within min(2 %, 3 cm), bearing 0.1 .. 0.3 rad either way, or the edge the case asks for (a whole number of turns on top, or an unwrapped
residual of +-(pi - 1e-5)).  The scripts are data afterwards: the model, the oracle and every device path read the same numbers.

Exact-boundary scripts (at most 8): theta = 0, eleven straight steps of binary-fraction lengths without an observation, then ONE
observation of a landmark on the robot's negative x axis with bearing 0 or +-2 pi_d: every operation is exact, atan2 returns pi_d
and the wrap's argument is an exact multiple of pi_d.  They are judged on the logged y alone.
"""
import dataclasses
import itertools

import numpy as np

from oracle import ekf_oracle as orc
from tests.streams import dense_start

N, NS, K = 12, 27, 12
THR = 1e-2
NX = float(np.nextafter(THR, 1.0))
UNDER = THR * (1 - 1e-12)
THR_WIDE = 0.05
NX_WIDE = float(np.nextafter(THR_WIDE, 1.0))
UNDER_WIDE = THR_WIDE * (1 - 1e-12)
TURN = 2 * np.pi
EDGE = np.pi - 1e-5

# The bars of the GPU module (tests/test_gpu_geometry.py) and of the mutants' judge (tests/test_geometry_cpu.py): distance from the
# longdouble model, y and pose absolute, S, NIS and the blocks relative.  Each is 16 x the larger of the worst device figure over
# every path and the float64 oracle's own distance (device atan2, sincos and rsq may sit a few ulp from glibc's), rounded up, and
# never above the project's 1e-9: profiles/geometry_edges.txt holds the measurement.  (H is not logged by the device: the
# oracle's and its mutants' are held to the bar of S, which H makes.)
DEVICE_TOL = 1e-9
DEVICE_BARS = dict(y=3.4e-11, S=8.6e-11, nis=8.0e-11, H=8.6e-11, pose=2.1e-12, pose_block=3.8e-12, state=3.1e-11,
                   state_entry=7.1e-10)
ASSOCIATE_BARS = dict(nis=2.4e-10, logdet=1.2e-10)         # associate(full=True): every pair's NIS relatively; over max(|ln det S|, 1)
TAGS_BAR = 9.1e-13                                         # tags_positions(): world guess, range and bearing, absolute
assert max(DEVICE_BARS.values()) <= DEVICE_TOL and max(ASSOCIATE_BARS.values()) <= DEVICE_TOL

RANGES = (1e-4, 1e-3, 0.3, 50.0, 1e4)
DIRS = (0.0, 1.0, np.pi / 2, -2.5, np.pi - 1e-6, -(np.pi - 1e-6))
COMBOS = [(RANGES[c % 5], DIRS[c % 6]) for c in range(30)]           # (5 and 6 are coprime: every pair once)
# Where a range may stand, so that float64 itself stays within the CPU module's conditions (profiles/geometry_edges.txt):
#   NEAR  millimetres: H's relative error is the pose's absolute error over the range, so only the first update of a script, where
#         the pose is one rounding from exact (2e-17 at |x| < 0.13: 2e-13 of 1e-4 m);
#   FAR   kilometres: d = l - x rounds at ulp(1e4) / 2 = 9e-13, which a gain of 0.2 carries into the pose and from there into
#         every later innovation -- unless the landmark starts at variance 1e4 and takes the whole innovation itself: the
#         landmarks observed once (ONCE), in a diagonal start;
#   MID   0.3 and 50 m: anywhere.
NEAR = [(RANGES[c % 2], DIRS[(c // 2 + 3 * (c % 2)) % 6]) for c in range(12)]
FAR = [(RANGES[2 + c % 3], DIRS[(c // 3 + 2 * (c % 3)) % 6]) for c in range(18)]
MID = [(RANGES[2 + c % 2], DIRS[(c // 2 + 3 * (c % 2)) % 6]) for c in range(12)]
EXTRAS = (0.0, 0.3, -0.3, TURN + 0.1, -2 * TURN - 0.2, EDGE, -EDGE)
EXTRAS_FAR_THETA = (0.0, 0.3, -0.3, EDGE, -EDGE)     # at theta = -1000 (ulp 1.1e-13) a residual of 0.1 cannot carry the NIS to 1e-12

ORDER = ((0, 1, 2, 3), (1, 0, 4, 2), (2, 4, 0, 1), (5, 2, 0, 4), (0, 5, 1, 2), (1, 6, 4, 5),
         (6, 0, 1, 2), (2, 4, 5, 7), (5, 6, 0, 1), (2, 6, 4, 5), (8, 6, 9, 4), (10, 6, 5, 11))
ONCE = (3, 7, 8, 9, 10, 11)        # observed exactly once: the landmarks that start at variance 1e4 in a diagonal start

LINS = (0.0, -0.12, 0.5, -0.5, 0.0, 0.12, 0.5, -0.12, 0.0, 0.5, -0.5, 0.12)
MOT_EDGES = (0.0, -THR, NX, -NX, UNDER, THR, 0.3, -0.3, 2.0, -7.0, NX, -THR)
MOT_UP = (0.3, -0.3, 0.3, THR, -0.3, -NX, 0.3, 2.0, -7.0, -0.3, -7.0, 2.0)            # from 3.1: over +pi, back over -pi, ...
MOT_DOWN = (-0.3, 0.3, -0.3, -THR, 0.3, NX, -0.3, 2.0, 2.0, 2.0, 2.0, -7.0)           # from -3.1; step 10 crosses +pi
MOT_FAR = (THR, 0.0, -THR, UNDER, -0.3, NX, 0.3, -NX, 2.0, THR, -7.0, 0.3)            # theta stays far outside for four steps; at
#                                                       theta = -1000 (turn = 0) the first arc has lin = 0 (r sin(theta + ang) at ulp(1000))
MOT_FAR_BRIEF = (THR, -7.0, NX, -0.3, 0.0, 2.0, UNDER, -NX, 0.3, -THR, -0.3, -7.0)     # one step far outside, then r = 0.017
MOT_MILD = (0.3, -THR, NX, -0.3, 0.0, 2.0, UNDER, -NX, 0.3, THR, -0.3, -7.0)
MOT_WIDE = (0.0, -THR_WIDE, NX_WIDE, -NX_WIDE, UNDER_WIDE, THR, -NX, 0.3, -0.3, 2.0, -7.0, THR_WIDE)
MOT_RUNAWAY = (-7.0, -7.0, -7.0, -7.0, -7.0, 0.3, -THR, NX, 2.0, -0.3, 2.0, -7.0)     # linear mode: theta = -38.1 before step 5


def lins_of(turn):
    """The script's lin per step: step 0 keeps lin = 0 (the pose its first update sees is the start itself), steps 1..11 take LINS
    turned by `turn` places, so that over the table every edge of ang meets lin of both signs and 0."""
    rest = LINS[1:]
    return (LINS[0],) + tuple(rest[(i + turn) % len(rest)] for i in range(len(rest)))


@dataclasses.dataclass
class Script:
    name: str
    cfg: orc.EkfConfig
    mean0: np.ndarray
    cov0: np.ndarray
    steps: list                    # [(lin, ang, [(landmark, range, bearing), ...])]
    exact: bool = False            # the last observation of the last step is an exact-boundary one
    edges: list = dataclasses.field(default_factory=list)     # [(step, position, what)]: where the case's edges sit

    @property
    def updates(self):
        return sum(len(o) for _, _, o in self.steps)


def start_cov(kind, seed):
    """diag: pose 0.1, landmarks 1e4 (ONCE) and 0.05^2 (the others); dense: streams.dense_start."""
    if kind == "dense":
        return dense_start(NS, seed)
    d = np.full(NS, 1e4)
    d[0:3] = 0.1
    for j in set(range(N)) - set(ONCE):
        d[3 + 2 * j:5 + 2 * j] = 0.05 ** 2
    return np.diag(d)


def build(name, theta0, angs, cov, seed, cfg=None, places=None, extras=None, cut=False, quiet_until=0, xy0=(0.003, -0.002), near=0,
          dr=(0.05, 0.15), draw=(0.2, 0.3), turn=None):
    """One script.  `places`: per landmark (range, world direction) of its first observation (default: 0.3 .. 1.95 m around the
    compass, and NEAR[near] for the script's first update); `extras`: (step, position) -> what the bearing gets on top of the true
    one (default: a draw of 0.2 .. 0.3 rad either way; the range residual is `dr` = 0.05 .. 0.15 m either way but at most half the
    range, a fifth of a millimetre range, 4 m of a kilometre range, whose y_0 float64 holds to 9e-13 only: innovations a relative
    bound on the NIS can be held against).  Step 0 has lin = 0: the pose the script's first update sees is the start itself."""
    cfg = cfg or orc.EkfConfig()
    rng = np.random.default_rng(seed)
    lins = lins_of(seed % (K - 1) if turn is None else turn)
    if places is None:
        places = [(0.3 + 0.15 * j, -2.5 + 0.5 * j) for j in range(N)]
        if near is not None:
            places[ORDER[0][0]] = NEAR[near % len(NEAR)]
    mean0 = np.zeros(NS)
    mean0[0:3] = (xy0[0], xy0[1], theta0)
    cov0 = start_cov(cov, seed)
    om, oP = mean0.copy(), cov0.copy()
    placed = [False] * N
    steps, edges = [], []
    for k in range(K):
        om, oP = orc.predict_dense(om, oP, lins[k], angs[k], cfg)
        obs = []
        order = ORDER[k][:3] if cut and k == 3 else ORDER[k]
        for i, j in enumerate(order if k >= quiet_until else ()):
            t = 3 + 2 * j
            if not placed[j]:
                r, phi = places[j]
                delta = om[0:2] + r * np.array([np.cos(phi), np.sin(phi)]) - om[t:t + 2]
                om[t:t + 2] += delta
                mean0[t:t + 2] += delta
                placed[j] = True
                edges.append((k, i, f"first observation at {r:g} m, world direction {phi:.6f}"))
            d = om[t:t + 2] - om[0:2]
            r = float(np.hypot(d[0], d[1]))
            true_b = float(orc.wrap_pi(np.arctan2(d[1], d[0]) - om[2]))
            extra = extras(k, i) if extras is not None else None
            if extra is None:
                extra = float(rng.uniform(*draw) * rng.choice([-1.0, 1.0]))
            else:
                edges.append((k, i, f"bearing {extra:+.6f} on the true one"))
            zr = r + float(rng.choice([-1.0, 1.0])) * (0.2 * r if r < 0.01 else 4.0 if r > 1e3 else min(0.5 * r, float(rng.uniform(*dr))))
            zb = true_b + extra
            if cfg.enable_measurement_model:
                om, oP = orc.update_dense(om, oP, [j], [zr], [zb], cfg)
            obs.append((j, zr, zb))
        steps.append((lins[k], angs[k], obs))
    return Script(name, cfg, mean0, cov0, steps, False, edges)


def first_place(what):
    """(range, world direction) out of an edge's description."""
    parts = what.replace("first observation at ", "").replace(" m, world direction", "").split()
    return float(parts[0]), float(parts[1])


def cycle_extras(shift, table=EXTRAS):
    return lambda k, i: table[(4 * k + i + shift) % len(table)]


def combos(v, dense=False, near=True):
    """Variant v of the first observations' (range, direction): NEAR for the script's first update, FAR for the landmarks observed
    once (50 m where a dense start would let a kilometre into the pose), MID for the others; the variants rotate the lists."""
    places = [None] * N
    first = ORDER[0][0]
    places[first] = NEAR[v % len(NEAR)] if near else MID[v % len(MID)]
    for o, j in enumerate(ONCE):
        r, phi = FAR[(6 * v + o + v // 3) % len(FAR)]
        places[j] = (50.0 if dense and r > 50.0 else r, phi)
    for p_, j in enumerate(j for j in range(N) if j not in ONCE and j != first):
        places[j] = MID[(5 * v + p_) % len(MID)]
    return places


def exact_script(name, x_l, var, bearing, lins):
    """theta = 0, y = 0, eleven straight steps (ang = 0) of binary-fraction lengths, then one observation of landmark 5 at
    (x_l, 0), x_l behind the robot: d_y = 0 exactly, atan2 = pi_d, residual bearing - pi_d."""
    cfg = orc.EkfConfig()
    mean0 = np.zeros(NS)
    mean0[0:3] = (0.25, 0.0, 0.0)
    mean0[13:15] = (x_l, 0.0)
    d = np.full(NS, 1e4)
    d[0:3] = 0.1
    d[13:15] = var
    x = 0.25 + sum(lins)
    assert x_l < x - 0.5
    steps = [(lins[k], 0.0, []) for k in range(K - 1)] + [(lins[K - 1], 0.0, [(5, (x - x_l) + 0.015625, bearing)])]
    return Script(name, cfg, mean0, np.diag(d), steps, True, [(K - 1, 0, f"exact boundary, bearing {bearing!r}")])


EXACT_LINS = (0.5, -0.25, 0.125, 0.5, 0.0, 0.25, -0.5, 0.125, 0.5, 0.25, -0.125, 0.5)


def make_banks():
    """[(bank name, [Script, ...])], every script of a bank under one config."""
    C = orc.EkfConfig
    default = [
        build("motion edges from theta 0", 0.0, MOT_EDGES, "diag", 1, near=6),
        build("over +pi from 3.1", 3.1, MOT_UP, "dense", 2, near=7),
        build("over -pi from -3.1, step 10 cut", -3.1, MOT_DOWN, "diag", 3, cut=True, near=8),
        build("theta 40 set through set_state", 40.0, MOT_FAR, "diag", 4, near=9),
        build("theta -1000 set through set_state", -1000.0, MOT_FAR, "dense", 5, near=10, dr=(0.3, 0.5), draw=(0.6, 0.9), turn=0),
        build("ranges and directions 0, theta 0", 0.0, MOT_MILD, "diag", 6, places=combos(0), extras=cycle_extras(0)),
        build("ranges and directions 1, theta 3.1", 3.1, MOT_MILD, "dense", 7, places=combos(1, True), extras=cycle_extras(3)),
        build("ranges and directions 2, theta -1000", -1000.0, MOT_FAR_BRIEF, "diag", 8, places=combos(2),
              extras=cycle_extras(5, EXTRAS_FAR_THETA), dr=(0.3, 0.5)),
        build("ranges and directions 3, theta 40, step 10 cut", 40.0, MOT_FAR, "dense", 9, places=combos(3, True),
              extras=cycle_extras(1), cut=True),
        build("ranges and directions 4, theta -3.1", -3.1, MOT_DOWN, "diag", 10, places=combos(4), extras=cycle_extras(2)),
        build("bearing edges at tame ranges, theta 0", 0.0, MOT_EDGES, "dense", 11, extras=cycle_extras(4), near=11),
    ]
    boundary = [exact_script(f"exact boundary, landmark at {x_l:g}, bearing {name}", x_l, var, b, EXACT_LINS)
                for x_l, var in ((-0.75, 0.05 ** 2), (-4096.0, 1e4))
                for name, b in (("0", 0.0), ("+2 pi_d", TURN), ("-2 pi_d", -TURN))]
    boundary += [
        build("motion edges from theta 0, dense, step 10 cut", 0.0, MOT_EDGES, "dense", 12, cut=True, near=0, turn=3),
        build("bearing edges from -3.1", -3.1, MOT_UP, "dense", 13, extras=cycle_extras(6), near=1),
    ]
    wide = C(arc_threshold=THR_WIDE)
    wide_bank = [
        build("threshold 0.05: its own edges", 0.0, MOT_WIDE, "diag", 14, cfg=wide, near=2, turn=9),
        build("threshold 0.05: ranges and directions, theta 3.1", 3.1, MOT_WIDE, "dense", 15, cfg=wide, places=combos(5, True),
              turn=10, extras=cycle_extras(0)),
        build("threshold 0.05: the default threshold's edges go straight", -3.1, MOT_EDGES, "diag", 16, cfg=wide, cut=True, near=3),
    ]
    nomeas = C(enable_measurement_model=False)
    nomeas_bank = [
        build("no measurement model: motion edges", 0.0, MOT_EDGES, "diag", 17, cfg=nomeas),
        build("no measurement model: over +pi from 3.1", 3.1, MOT_UP, "dense", 18, cfg=nomeas),
    ]
    nomotion = C(disable_motion_model=True)
    nomotion_bank = [
        build("no motion model: ranges and directions, theta 40", 40.0, MOT_EDGES, "diag", 19, cfg=nomotion, places=combos(6, near=False),
              extras=cycle_extras(2)),
        build("no motion model: theta -3.1", -3.1, MOT_UP, "dense", 20, cfg=nomotion, extras=cycle_extras(5), near=None),
    ]
    linear = C(enable_circular_interpolation=False)
    linear_bank = [
        build("linear mode: theta 40, ranges and directions", 40.0, MOT_FAR, "diag", 21, cfg=linear, places=combos(7),
              extras=cycle_extras(1)),
        build("linear mode: theta runs away to -38 unobserved", -3.1, MOT_RUNAWAY, "dense", 22, cfg=linear, quiet_until=5, near=None,
              extras=cycle_extras(3)),
        build("linear mode: motion edges", 0.0, MOT_EDGES, "diag", 23, cfg=linear, cut=True, near=4),
    ]
    return [("default", default), ("boundary", boundary), ("threshold", wide_bank), ("no_measurement", nomeas_bank),
            ("no_motion", nomotion_bank), ("linear", linear_bank)]


_BANKS = None


def banks():
    """The table, built once."""
    global _BANKS
    if _BANKS is None:
        _BANKS = make_banks()
        for _, scripts in _BANKS:
            assert 2 <= len(scripts) <= 16 and all(s.cfg == scripts[0].cfg for s in scripts)
    return _BANKS


BANK_NAMES = ("default", "boundary", "threshold", "no_measurement", "no_motion", "linear")


def bank(name):
    return dict(banks())[name]


def stacked(scripts):
    """A bank's scripts as stream_upload takes them: lin, ang (K, B); idx, zr, zb (K, B, 4); m (K, B)."""
    B = len(scripts)
    lin, ang = np.zeros((K, B)), np.zeros((K, B))
    idx, zr, zb = np.zeros((K, B, 4), dtype=np.int32), np.zeros((K, B, 4)), np.zeros((K, B, 4))
    m = np.zeros((K, B), dtype=np.int32)
    for b, s in enumerate(scripts):
        for k, (l, a, obs) in enumerate(s.steps):
            lin[k, b], ang[k, b], m[k, b] = l, a, len(obs)
            for i, (j, r, brg) in enumerate(obs):
                idx[k, b, i], zr[k, b, i], zb[k, b, i] = j, r, brg
    return lin, ang, idx, zr, zb, m


def step_args(scripts, k):
    """Step k of a bank as step() / update() take it: lin (B,), ang (B,), and per trajectory the lists of idx, ranges, bearings."""
    lin = np.array([s.steps[k][0] for s in scripts])
    ang = np.array([s.steps[k][1] for s in scripts])
    obs = [s.steps[k][2] for s in scripts]
    return (lin, ang, [np.array([o[0] for o in ob], dtype=np.int32) for ob in obs], [[o[1] for o in ob] for ob in obs],
            [[o[2] for o in ob] for ob in obs])


ASSOCIATE_SHIFT = (0.07, 0.05)


def association_observations(script):
    """What associate() is asked to score behind a script: the last step's ranges and bearings moved by 7 cm and 0.05 rad.  (The
    measurements themselves have just been applied: a landmark that started at 1e4 then sits on its own, and its pair's NIS of
    ~1e-11 from y ~ 1e-6 is a figure no arithmetic holds relatively.)"""
    obs = script.steps[-1][2]
    return [o[1] + ASSOCIATE_SHIFT[0] for o in obs], [o[2] + ASSOCIATE_SHIFT[1] for o in obs]


# ---- detections ---------------------------------------------------------------------------------------------------------------
def detection_windows():
    """Three trajectories, four windows each, as step_detections takes them: [(lin, ang, [window per trajectory])], the tags given
    by (id, x, z) in the camera frame (range^2 = x^2 + z^2 inside gate_range = 1.5; robot frame x_r = z, y_r = -x): ahead (z > 0
    near the axis), abeam (z ~ 0, either side) and behind (z < 0, off the axis, either side: bearings beyond +-pi/2 up to
    +-3.1)."""
    ahead = [(0, 0.05, 1.2), (1, -0.3, 0.9), (2, 0.0, 0.4)]
    abeam = [(3, 0.8, 1e-3), (4, -1.1, -1e-3), (5, 0.5, 0.0)]
    behind = [(6, 0.05, -1.2), (7, -0.04, -0.9), (8, 0.6, -0.7), (9, -0.9, -0.3)]
    sets = [ahead + behind[:2], abeam + behind[2:], behind + ahead[:1] + abeam[:1]]
    motions = [(0.12, 0.3), (0.5, -NX), (-0.12, THR), (0.12, -7.0)]
    out = []
    for k, (lin, ang) in enumerate(motions):
        wins = []
        for b in range(3):
            tags = sets[(b + k) % 3]
            jitter = 0.003 * (k + 1) * (1 if b % 2 else -1)
            wins.append([(float(k), [(i, x + jitter, z - jitter) for i, x, z in tags]),
                         (k + 0.1, [(i, x - jitter, z + 0.5 * jitter) for i, x, z in tags[:3]])])
        out.append((lin, ang, wins))
    return out


def tag_objects(win):
    """A window of (id, x, z) tuples as the reference's detections: [(stamp, [tag, ...])]."""
    from types import SimpleNamespace as NS
    return [(stamp, [NS(tag_id=i, pose_R=np.eye(3), pose_t=np.array([[x], [0.0], [z]]), pose_err=0.0) for i, x, z in tags])
            for stamp, tags in win]


DET_START = (np.zeros(3), np.eye(3) * 0.1)


class DetectionReference:
    """One trajectory of detection_windows() through the oracle's association and augmentation (float64: averaging, range,
    bearing, world guess -- orc.associate / orc.augment) and the longdouble step: per window the oracle's tags_positions and
    the step's record, and the final state."""

    def __init__(self):
        self.tags, self.recs, self.mean, self.cov = [], [], None, None


def detection_reference():
    from tests import geometry_model as gm
    cfg = orc.EkfConfig()
    out = []
    for b in range(3):
        ref = DetectionReference()
        mean, cov, index = gm.ld(DET_START[0]), gm.ld(DET_START[1]), {}
        for lin, ang, wins in detection_windows():
            tags = orc.associate(tag_objects(wins[b]), index, mean[0:3].astype(np.float64), cfg)
            n_old, n_new = len(mean), 3 + 2 * len(index)
            grown, gcov = np.zeros(n_new, dtype=gm.LD), np.zeros((n_new, n_new), dtype=gm.LD)
            grown[:n_old], gcov[:n_old, :n_old] = mean, cov
            for i in range(n_old, n_new, 2):                       # orc.augment (:341-360)
                j = (i - 3) // 2
                grown[i], grown[i + 1] = tags[j][0], tags[j][1]
                gcov[i, i] = gcov[i + 1, i + 1] = cfg.landmark_init_var
            rec = gm.StepRecord()
            mean, cov = gm.step(grown, gcov, lin, ang, [(j, tags[j][4], tags[j][5]) for j in tags], cfg, rec)
            ref.tags.append(tags)
            ref.recs.append(rec)
        ref.mean, ref.cov = mean, cov
        out.append(ref)
    return out


def all_scripts():
    return list(itertools.chain.from_iterable(s for _, s in banks()))
