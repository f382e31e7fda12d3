"""The inputs and the oracle shared by tests/test_transport.py (CPU) and tests/test_transport_gpu.py: the optimal partition of
a track into diffusive and directed stretches BY DEFINITION, a plain double loop over (i, j) in Python floats, written from
include/mivit_hip.h (mivit_segment_transport) and not from helpers/msd._transport_numpy.

Tolerance of the cost (COST_RTOL): as in tests/segment_common.py, the only operation of the recurrence that may differ between
the kernel, numpy and math.log is log, at about 1 ulp (1.1e-16 relative on each term 2 n log(.)).  A candidate now takes TWO
logs (C0 and C1), but a term of F is the lower of the two, so one log's error enters a term; the other can at most swap which
of two nearly equal costs is taken, which moves the term by no more than that error again: 2.2e-16 relative per term.  F(Linc)
sums at most 512 terms on the tracks below (513 rows): 512 * 2.2e-16 * |cost| = 1.1e-13 relative if every error had the same
sign; 1e-10 * (1 + |cost|) leaves a factor of 900.  The one track of ops.TRANSPORT_MAX_LEN rows of the GPU test has 4095
terms: 9e-13, a factor of 100.

Margins: the smallest over the backtracked path of the gap between the chosen candidate and the runner-up and (mode "both") of
|C0 - C1| at the chosen candidate is at least MIN_MARGIN = 1e-6 on every track below in every mode (tests/test_transport.py
asserts it; the seed was picked so that the restatement holds it), seven orders above the rounding of F, so the kernel's
partition AND classes must equal the restatement's on EVERY track."""
import functools
import math

import numpy as np

MIN_LEN = 4
PENALTY = 3.0
VELOCITY_PENALTY = 3.0
MIN_VAR = 1e-12
COST_RTOL = 1e-10
MIN_MARGIN = 1e-6
D_LOW = 0.05
STEP_SD = math.sqrt(2.0 * D_LOW)                                           # of one axis of one increment
FIXED_LENGTHS = (1, 2, 3, 2 * MIN_LEN, 2 * MIN_LEN + 1, 64, 65, 66, 257, 513)
MODES = {"both": 0, "directed": 1, "diffusive": 2}
SEED = 20250310


def brownian(rng, rows, D):
    """[rows, 2] positions with per-axis step variance 2 D."""
    steps = rng.standard_normal((rows, 2)) * math.sqrt(2.0 * D)
    steps[0] = 0.0
    return np.cumsum(steps, axis=0) + 20.0


def run_and_pause(rng, n_changes, speed, stretch, start_run=False, D=D_LOW):
    """A track of n_changes + 1 stretches of `stretch` increments that alternate pause and run at one D: a run moves at `speed`
    step standard deviations per frame in a direction drawn per run -> (positions [rows, 2], the planted cuts as increment
    indices, the class of every stretch, the velocity (y, x) of every stretch)."""
    sd = math.sqrt(2.0 * D)
    classes = [(s + (1 if start_run else 0)) % 2 for s in range(n_changes + 1)]
    vel = []
    for c in classes:
        phi = rng.uniform(0.0, 2.0 * math.pi)
        vel.append((c * speed * sd * math.sin(phi), c * speed * sd * math.cos(phi)))
    drift = np.repeat(np.array(vel), stretch, axis=0)
    steps = np.concatenate([np.zeros((1, 2)), rng.standard_normal((len(drift), 2)) * sd + drift])
    return np.cumsum(steps, axis=0) + 20.0, [stretch * (s + 1) for s in range(n_changes)], classes, vel


@functools.lru_cache(maxsize=None)
def common_tracks():
    """-> (pos [N, 2] float64, offsets [n_tracks + 1] int64, planted: {track index: (cuts, classes)}), read-only."""
    rng = np.random.default_rng(SEED)
    tracks, plant = [], {}
    for L in FIXED_LENGTHS:
        tracks.append(brownian(rng, L, 0.3))
    tracks.insert(5, np.zeros((0, 2)))                                     # an empty track in the middle of the batch
    tracks.append(np.full((20, 2), 7.25))                                  # never moves: the min_var floor in both costs
    for speed in (3.0, 1.5):
        for stretch in (30, 60):
            for n_changes in (0, 1, 3):
                p, cuts, classes, _ = run_and_pause(rng, n_changes, speed, stretch, start_run=stretch == 60)
                plant[len(tracks)] = (cuts, classes)
                tracks.append(p)
    pos = np.ascontiguousarray(np.concatenate(tracks, axis=0))
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    pos.setflags(write=False)
    offsets.setflags(write=False)
    return pos, offsets, plant


N_TRACKS = len(FIXED_LENGTHS) + 2 + 12


def _sums(p):
    cs2, csy, csx = [0.0], [0.0], [0.0]
    for k in range(len(p) - 1):
        dy, dx = float(p[k + 1, 0]) - float(p[k, 0]), float(p[k + 1, 1]) - float(p[k, 1])
        cs2.append(cs2[-1] + (dy * dy + dx * dx) if k else dy * dy + dx * dx)
        csy.append(csy[-1] + dy if k else dy)
        csx.append(csx[-1] + dx if k else dx)
    return cs2, csy, csx


def _cost(sums, i, j, min_var, gamma, mode):
    """(C, class) of the stretch (i, j) as include/mivit_hip.h defines them."""
    cs2, csy, csx = sums
    n = j - i
    tn = 2.0 * n
    SS, Sy, Sx = cs2[j] - cs2[i], csy[j] - csy[i], csx[j] - csx[i]
    C0 = tn * math.log(max(SS / tn, min_var))
    C1 = tn * math.log(max((SS - (Sy * Sy + Sx * Sx) / n) / tn, min_var)) + gamma
    if mode == 1:
        return C1, 1
    if mode == 2:
        return C0, 0
    return (C1, 1) if C1 < C0 else (C0, 0)


def oracle_track(p, mode, min_len=MIN_LEN, penalty=PENALTY, velocity_penalty=VELOCITY_PENALTY, min_var=MIN_VAR):
    """One track [rows, 2] -> (cuts: ascending increment indices, the class of every stretch, cost F(Linc); NaN and no stretch
    without an increment)."""
    Linc = len(p) - 1
    if Linc < 1:
        return [], ([0] if len(p) == 1 else []), float("nan")
    sums = _sums(p)
    lg = math.log(float(Linc))
    beta, gamma = penalty * lg, velocity_penalty * lg
    F, prev = {0: -beta}, {}
    if Linc < min_len:
        C, cls = _cost(sums, 0, Linc, min_var, gamma, mode)
        return [], [cls], (F[0] + C) + beta
    for j in range(min_len, Linc + 1):
        best, arg = math.inf, (0, 0)
        for i in [0] + list(range(min_len, j - min_len + 1)):
            C, cls = _cost(sums, i, j, min_var, gamma, mode)
            v = (F[i] + C) + beta
            if v < best:
                best, arg = v, (i, cls)
        F[j], prev[j] = best, arg
    cuts, classes, j = [], [], Linc
    while j > 0:
        j, cls = prev[j]
        classes.append(cls)
        if j > 0:
            cuts.append(j)
    return cuts[::-1], classes[::-1], F[Linc]


def score_partition(p, cuts, classes, mode, penalty=PENALTY, velocity_penalty=VELOCITY_PENALTY, min_var=MIN_VAR):
    """The penalised cost of a GIVEN partition with GIVEN classes: what the oracle's optimum is a lower bound of."""
    Linc = len(p) - 1
    sums = _sums(p)
    lg = math.log(float(Linc))
    edges = [0] + list(cuts) + [Linc]
    total = lg * penalty * len(cuts)
    for a, b, c in zip(edges[:-1], edges[1:], classes):
        total += _cost(sums, a, b, min_var, velocity_penalty * lg, 1 if c else 2)[0]
    return total


@functools.lru_cache(maxsize=None)
def oracle_common(mode):
    """-> (list of cut lists, list of class lists, cost [n_tracks]) of common_tracks() in one mode (0, 1 or 2), computed once."""
    pos, offsets, _ = common_tracks()
    out = [oracle_track(pos[a:b], mode) for a, b in zip(offsets[:-1], offsets[1:])]
    cost = np.array([c for _, _, c in out])
    cost.setflags(write=False)
    return [c for c, _, _ in out], [c for _, c, _ in out], cost


def partition_of(seg_start, seg_class, offsets):
    """seg_start, seg_class [N] and the track CSR -> per track (cuts as increment indices, the class of every stretch); checks
    that the class is constant over a stretch."""
    cuts, classes = [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        s, c = np.asarray(seg_start[a:b]), np.asarray(seg_class[a:b])
        r = np.nonzero(s)[0]
        if b > a:
            assert r[0] == 0, "the first row of a track starts a stretch"
        assert set(np.unique(c).tolist()) <= {0, 1}
        edges = list(r) + [b - a]
        for lo, hi in zip(edges[:-1], edges[1:]):
            assert (c[lo:hi] == c[lo]).all(), "one class per stretch"
        cuts.append([int(v) for v in r[1:]])
        classes.append([int(c[v]) for v in r])
    return cuts, classes


def direct_stats(p, dt, R):
    """(velocity (y, x), D_res, D_cve, sigma2) of the increments of one stretch [rows, 2], straight from the formulas."""
    d = np.diff(np.asarray(p, np.float64), axis=0)
    n = len(d)
    if n < 1:
        return (math.nan, math.nan), math.nan, math.nan, math.nan
    m = d.mean(axis=0)
    e = d - m
    S2 = float((e ** 2).sum())
    S11 = float((e[:-1] * e[1:]).sum())
    res = S2 / (4 * n * dt)
    if n < 2:
        return (m[0] / dt, m[1] / dt), res, math.nan, math.nan
    return (m[0] / dt, m[1] / dt), res, res + S11 / (2 * (n - 1) * dt), R * S2 / (2 * n) + (2 * R - 1) * S11 / (2 * (n - 1))


def planted_path(n_particles, n_frames, switch):
    """[n_particles, n_frames] int64 state path: even particles pause (state 0) before frame `switch` and run (state 1) from
    it, odd ones the reverse."""
    path = np.zeros((n_particles, n_frames), np.int64)
    path[0::2, switch:] = 1
    path[1::2, :switch] = 1
    return path
