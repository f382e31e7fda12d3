"""The inputs and the oracle shared by tests/test_segment.py (CPU) and tests/test_segment_gpu.py: the optimal partition of a
track into stretches of constant step variance BY DEFINITION, a plain double loop over (i, j) in Python floats, written from
include/mivit_hip.h and not from helpers/msd._segment_numpy.

Tolerance of the cost (COST_RTOL): the only operation of the recurrence that may differ between the kernel and numpy is log, at
about 1 ulp (1.1e-16 relative on each term 2 n log(.)).  F(Linc) sums at most 512 such terms on the tracks below (513 rows),
so the two differ by about 512 * 1.1e-16 * |cost| = 5e-13 relative if every error had the same sign; 1e-10 * (1 + |cost|)
leaves a factor of 200.

Margins: the smallest gap between the chosen candidate and the runner-up on the backtracked path, per track, is at least
MIN_MARGIN = 1e-6 on every track below (tests/test_segment.py asserts it), seven orders above the rounding of F, so the
kernel's partition must equal the restatement's on EVERY track."""
import functools
import math

import numpy as np

MIN_LEN = 4
PENALTY = 3.0
MIN_VAR = 1e-12
COST_RTOL = 1e-10
MIN_MARGIN = 1e-6
D_LOW = 0.05
FIXED_LENGTHS = (1, 2, 3, 2 * MIN_LEN, 2 * MIN_LEN + 1, 64, 65, 66, 257, 513)


def brownian(rng, rows, D):
    """[rows, 2] positions with per-axis step variance 2 D."""
    steps = rng.standard_normal((rows, 2)) * math.sqrt(2.0 * D)
    steps[0] = 0.0
    return np.cumsum(steps, axis=0) + 20.0


def planted(rng, n_changes, ratio, stretch):
    """A track of n_changes + 1 stretches of `stretch` increments whose D alternates between D_LOW and ratio * D_LOW ->
    (positions [rows, 2], the planted changepoints as increment indices)."""
    Ds = [D_LOW if s % 2 == 0 else D_LOW * ratio for s in range(n_changes + 1)]
    scale = np.repeat(np.sqrt(2.0 * np.array(Ds)), stretch)
    steps = np.concatenate([np.zeros((1, 2)), rng.standard_normal((len(scale), 2)) * scale[:, None]])
    return np.cumsum(steps, axis=0) + 20.0, [stretch * (s + 1) for s in range(n_changes)]


@functools.lru_cache(maxsize=None)
def common_tracks():
    """-> (pos [N, 2] float64, offsets [n_tracks + 1] int64, planted: {track index: (ratio, [changepoints])}), read-only."""
    rng = np.random.default_rng(20240611)
    tracks, plant = [], {}
    for L in FIXED_LENGTHS:
        tracks.append(brownian(rng, L, 0.3))
    tracks.insert(5, np.zeros((0, 2)))                                     # an empty track in the middle of the batch
    tracks.append(np.full((20, 2), 7.25))                                  # never moves: the min_var floor
    for ratio in (20, 4):
        for stretch in (30, 60):
            for n_changes in (0, 1, 3):
                p, cps = planted(rng, n_changes, ratio, stretch)
                plant[len(tracks)] = (ratio, cps)
                tracks.append(p)
    pos = np.ascontiguousarray(np.concatenate(tracks, axis=0))
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    pos.setflags(write=False)
    offsets.setflags(write=False)
    return pos, offsets, plant


def _cs(p):
    cs = [0.0]
    for k in range(len(p) - 1):
        dy, dx = float(p[k + 1, 0]) - float(p[k, 0]), float(p[k + 1, 1]) - float(p[k, 1])
        cs.append(cs[-1] + (dy * dy + dx * dx) if k else dy * dy + dx * dx)
    return cs


def _cost(cs, i, j, min_var):
    tn = 2.0 * (j - i)
    return tn * float(np.log(max((cs[j] - cs[i]) / tn, min_var)))


def oracle_track(p, min_len=MIN_LEN, penalty=PENALTY, min_var=MIN_VAR):
    """One track [rows, 2] -> (changepoints: ascending increment indices, cost F(Linc); NaN without an increment)."""
    Linc = len(p) - 1
    if Linc < 1:
        return [], float("nan")
    cs = _cs(p)
    beta = penalty * float(np.log(float(Linc)))
    F, prev = {0: -beta}, {}
    if Linc < min_len:
        return [], (F[0] + _cost(cs, 0, Linc, min_var)) + beta
    for j in range(min_len, Linc + 1):
        best, arg = math.inf, 0
        for i in [0] + list(range(min_len, j - min_len + 1)):
            v = (F[i] + _cost(cs, i, j, min_var)) + beta
            if v < best:
                best, arg = v, i
        F[j], prev[j] = best, arg
    cps, j = [], Linc
    while j > 0:
        j = prev[j]
        if j > 0:
            cps.append(j)
    return cps[::-1], F[Linc]


def score_partition(p, cps, penalty=PENALTY, min_var=MIN_VAR):
    """The penalised cost of a GIVEN partition of one track: what the oracle's optimum is a lower bound of."""
    Linc = len(p) - 1
    cs = _cs(p)
    beta = penalty * float(np.log(float(Linc)))
    edges = [0] + list(cps) + [Linc]
    return sum(_cost(cs, a, b, min_var) for a, b in zip(edges[:-1], edges[1:])) + beta * len(cps)


@functools.lru_cache(maxsize=None)
def oracle_common():
    """-> (list of changepoint lists, cost [n_tracks]) of common_tracks(), computed once."""
    pos, offsets, _ = common_tracks()
    out = [oracle_track(pos[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    cost = np.array([c for _, c in out])
    cost.setflags(write=False)
    return [c for c, _ in out], cost


def changepoints_of(seg_start, offsets):
    """seg_start [N] and the track CSR -> per track the changepoints as increment indices (rows relative to the track)."""
    out = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        r = np.nonzero(np.asarray(seg_start[a:b]))[0]
        if b > a:
            assert r[0] == 0, "the first row of a track starts a segment"
        out.append([int(v) for v in r[1:]])
    return out


def direct_stats(p, dt, R):
    """(D_cve, D_mle, sigma2) of the increments of one stretch [rows, 2], straight from the formulas."""
    d = np.diff(np.asarray(p, np.float64), axis=0)
    n = len(d)
    S2 = float((d ** 2).sum())
    S11 = float((d[:-1] * d[1:]).sum())
    mle = S2 / (4 * n * dt) if n >= 1 else math.nan
    if n < 2:
        return math.nan, mle, math.nan
    return mle + S11 / (2 * (n - 1) * dt), mle, R * S2 / (2 * n) + (2 * R - 1) * S11 / (2 * (n - 1))


def markov_loop(u, p0, M):
    """The state path by a Python loop over particles and frames."""
    u, p0, M = np.asarray(u, np.float64), np.asarray(p0, np.float64), np.asarray(M, np.float64)
    K = len(p0)
    out = np.zeros(u.shape, np.int32)
    for n in range(u.shape[0]):
        row = p0
        for t in range(u.shape[1]):
            c, k = row[0], 0
            while k < K - 1 and not u[n, t] < c:
                k += 1
                c = c + row[k]
            out[n, t] = k
            row = M[k]
    return out
