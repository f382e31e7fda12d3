"""What tests/test_drift.py (CPU) and tests/test_drift_gpu.py share: ONE read-only common set for the drift kernels of
csrc/drift.hip and an INDEPENDENT oracle in plain Python (loops over tracks and frames, math.fsum for the mean, sorted for the
median), which knows nothing of the kernel's summation order.

The common table (common_table) is built of two-row tracks, one per wanted increment, in a shuffled track order, so that the
pairs of a frame are scattered over the table; FRAME_PAIRS says how many increments each frame must end up with.  It covers
frames of 0, 1, 2, 3, 63, 64, 65, 127, 128, 129 increments, 300 (above the 256 partial sums the mean takes in one pass, and a
padded sort of 512) and 257; two frames whose increments hold ties, -0 and +0 (4 and 5 increments); and the special tracks:
two tracks of 0 rows, one of 1 row, a track with a frame gap of 2, a track with a masked row, one with a NaN row and one with
an Inf row.  Frame 1 has one increment, so min_pairs = 2 empties it.

The integrate cases (integrate_case) are random stat / n_pairs of F = 1, 2, h, h + 1, 2 h + 1 (h = HALF_WINDOW), 257 (one
above the block of the running sum) and 65 793 (one above a block past the 65 536 frames one pass of the kernel takes), with
stretches of frames without pairs longer than a window."""
import functools
import math

import numpy as np

HALF_WINDOW = 3
INTEGRATE_F = (1, 2, HALF_WINDOW, HALF_WINDOW + 1, 2 * HALF_WINDOW + 1, 257, 65536 + 257)
# frame -> the used increments it must have (frame 0 can have none)
FRAME_PAIRS = {1: 1, 2: 2, 3: 3, 4: 63, 5: 64, 6: 65, 7: 127, 8: 128, 9: 129, 10: 300, 11: 0, 12: 4, 13: 5, 14: 0, 15: 0, 16: 1,
               17: 1, 18: 257}
N_FRAMES = 20                                                              # frame 19 has no row at all
TIE_FRAMES = (12, 13)
N_REJECTED = 3
# (y, x) increments of the tie frames, in track order: -0 comes from (-0) - (+0), +0 from (+0) - (+0)
TIES = {12: [(0.0, 0.5), (-0.0, 0.5), (0.0, -0.5), (-0.0, 0.5)],
        13: [(0.0, 0.25), (-0.0, 0.25), (1.0, 0.25), (-1.0, -3.0), (0.0, 7.0)]}
EPS = 2.0 ** -52


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def common_table():
    """-> (pos [N, 2] float64, frames [N] int64, offsets [n_tracks + 1] int64, use [N] bool), read-only."""
    rng = np.random.default_rng(20261019)
    tracks = []                                                            # (frames, positions, use) per track
    for f, c in FRAME_PAIRS.items():
        if f in TIE_FRAMES or f in (14, 15, 16, 17):
            continue
        for _ in range(c):
            p0 = rng.uniform(5.0, 60.0, 2)
            tracks.append(([f - 1, f], [p0, p0 + rng.normal(0.3, 0.7, 2)], [True, True]))
    for f in TIE_FRAMES:
        for dy, dx in TIES[f]:
            tracks.append(([f - 1, f], [np.array([0.0, 8.0]), np.array([dy, 8.0 + dx])], [True, True]))
    nan, inf = float("nan"), float("inf")
    tracks.append(([], [], []))                                            # no rows
    tracks.append(([5], [np.array([3.0, 4.0])], [True]))                   # one row
    tracks.append(([14, 16, 17], [np.array([1.0, 1.0]), np.array([9.0, 9.0]), np.array([9.5, 8.75])], [True] * 3))   # a gap of 2
    tracks.append(([14, 15, 16], [np.array([2.0, 2.0]), np.array([2.5, 2.5]), np.array([3.0, 3.5])], [True, False, True]))
    tracks.append(([14, 15, 16], [np.array([4.0, 4.0]), np.array([nan, 4.5]), np.array([5.0, 5.0])], [True] * 3))
    tracks.append(([15, 16, 17], [np.array([6.0, 6.0]), np.array([6.25, 5.5]), np.array([6.5, inf])], [True] * 3))
    tracks.append(([], [], []))
    order = rng.permutation(len(tracks))
    pos, frames, use, offsets = [], [], [], [0]
    for k in order:
        fr, p, u = tracks[k]
        frames += fr
        pos += [np.asarray(q, dtype=np.float64) for q in p]
        use += u
        offsets.append(len(frames))
    return (_ro(np.array(pos, dtype=np.float64).reshape(-1, 2)), _ro(np.array(frames, dtype=np.int64)),
            _ro(np.array(offsets, dtype=np.int64)), _ro(np.array(use, dtype=bool)))


def oracle_increments(pos, frames, offsets, use, n_frames, min_pairs=1):
    """-> (per frame the list of (dy, dx) in ascending row, n_rejected): the selection rule of estimate_drift, row by row."""
    per_frame = [[] for _ in range(n_frames)]
    rejected = 0
    for k in range(len(offsets) - 1):
        for r in range(int(offsets[k]) + 1, int(offsets[k + 1])):
            if int(frames[r]) - int(frames[r - 1]) != 1 or not (use[r] and use[r - 1]):
                continue
            if not all(math.isfinite(float(v)) for v in (*pos[r], *pos[r - 1])):
                rejected += 1
                continue
            per_frame[int(frames[r])].append((r, float(pos[r, 0]) - float(pos[r - 1, 0]), float(pos[r, 1]) - float(pos[r - 1, 1])))
    out = []
    for lst in per_frame:
        lst.sort(key=lambda e: e[0])
        out.append([(dy, dx) for _, dy, dx in lst] if len(lst) >= min_pairs else [])
    return out, rejected


def _total_order(v):
    return (v, math.copysign(1.0, v))                                      # -0 before +0, as the kernel's keys order them


def oracle_stat(increments, estimator):
    """-> (stat [F][2] floats, sum_abs [F][2]: the sum of |d| the mean's bound is made of)."""
    stat, sum_abs = [], []
    for lst in increments:
        row, ab = [0.0, 0.0], [0.0, 0.0]
        for axis in range(2):
            vals = [e[axis] for e in lst]
            ab[axis] = math.fsum(abs(v) for v in vals)
            if not vals:
                continue
            if estimator == "mean":
                row[axis] = math.fsum(vals) / len(vals)
            else:
                s = sorted(vals, key=_total_order)
                n = len(s)
                row[axis] = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0
        stat.append(row)
        sum_abs.append(ab)
    return stat, sum_abs


def oracle_integrate(stat, n_pairs, h):
    """-> (velocity, drift [F][2] floats, vel_bound, drift_bound [F][2]).  fsum is exact up to one rounding; the bounds say how
    far a sum of the same terms in ANY order may lie from it:  a sum of m terms differs from the exact one by at most
    (m - 1) 2^-53 sum|t| (1 + O(eps)), bounded here by m 2^-52 sum|t|; each product n * stat adds 2^-53 |t|, the division
    2^-53 |v|."""
    F = len(stat)
    vel = [[0.0, 0.0] for _ in range(F)]
    vb = [[0.0, 0.0] for _ in range(F)]
    for f in range(1, F):
        for axis in range(2):
            if h == 0:
                vel[f][axis] = stat[f][axis]
                continue
            win = range(max(1, f - h), min(F - 1, f + h) + 1)
            den = sum(int(n_pairs[g]) for g in win)
            if den == 0:
                continue
            terms = [float(int(n_pairs[g])) * stat[g][axis] for g in win]
            vel[f][axis] = math.fsum(terms) / den
            vb[f][axis] = (len(terms) + 1) * EPS * math.fsum(abs(t) for t in terms) / den + EPS * abs(vel[f][axis])
    drift, db = [], []
    for axis in range(2):
        col, bcol, run_abs, run_vb = [], [], 0.0, 0.0
        partial = [0.0]                                                    # an exact running sum (Shewchuk's partials)
        for f in range(F):
            partial = _grow(partial, vel[f][axis])
            run_abs += abs(vel[f][axis])
            run_vb += vb[f][axis]
            col.append(math.fsum(partial))
            bcol.append(run_vb + (f + 1) * EPS * run_abs * (1.0 + 1e-9))
        drift.append(col)
        db.append(bcol)
    return vel, [list(r) for r in zip(*drift)], vb, [list(r) for r in zip(*db)]


def _grow(partials, x):
    """math.fsum's step: add x to a list of non-overlapping partial sums without losing a bit."""
    out = []
    for y in partials:
        if abs(x) < abs(y):
            x, y = y, x
        hi = x + y
        lo = y - (hi - x)
        if lo:
            out.append(lo)
        x = hi
    out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def integrate_case(F):
    """-> (stat [F, 2] float64, n_pairs [F] int32), read-only: frames without pairs (stat 0 there, as drift_frames leaves it)
    alone and in a stretch of 2 h + 3 frames."""
    rng = np.random.default_rng(1000 + F)
    n = rng.integers(0, 6, F).astype(np.int32)
    if F > 40:
        n[20:20 + 2 * HALF_WINDOW + 3] = 0
    stat = rng.normal(0.2, 1.0, (F, 2)) * (n > 0)[:, None]
    return _ro(stat), _ro(n)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a
