"""Shared by tests/test_crowded_detection.py (CPU) and tests/test_crowded_detection_gpu.py: frames with hundreds to two
thousand peak candidates, built on the CPU, and their restated results.  Nothing here needs a GPU.

The handle on csrc/peaks.h: with w1 = [1.0], w2 = [0.0] (radii 0) the difference of Gaussians of mivit_dog_peaks is the movie
itself, bit for bit, so a test hands tk_mask_kernel / tk_select_kernel any map it likes.  Maps are 48 x 96 (3 x 2 tiles of
16 x 64, the right-hand tiles partial) of small integers in float32, below 4096, on a background of zeros: THRESHOLD = 2^-12
times the frame's maximum is an exact product that lies below 1, the smallest peak, and above 0 in every frame."""
import functools
from collections import namedtuple

import numpy as np

from lrt_common import CAMERA, camera_movie, restated_stage2
from moleculardiffusion_mivit_amd.helpers import tracking as T

H, W = 48, 96
THRESHOLD = 2.0 ** -12
IDENTITY = (np.array([1.0]), np.array([0.0]))                             # w1, w2 of the identity "filter"
SITES = np.array([(y, x) for y in range(0, H, 2) for x in range(0, W, 2)], np.int64)   # the spacing-2 lattice, row-major
CROWD = 1000                                                              # isolated peaks of the tie builders start here

# a peak-selection case: movie [F, 48, 96] float32 (read-only) and min_distance; pairs: the tie builders' own record
Case = namedtuple("Case", "name movie min_distance pairs")


def _done(name, movie, min_distance=1, pairs=()):
    movie = np.ascontiguousarray(movie, np.float32)
    assert movie.max() < 1.0 / THRESHOLD and movie.min() >= 0.0
    movie.setflags(write=False)
    return Case(name, movie, min_distance, tuple(pairs))


def lattice_frame(n, seed=0):
    """the first n sites of the spacing-2 lattice carry n of the values 1 .. 1152 in a seeded random order"""
    values = np.random.default_rng(seed).permutation(len(SITES)) + 1
    m = np.zeros((H, W), np.float32)
    m[SITES[:n, 0], SITES[:n, 1]] = values[:n]
    return m


@functools.lru_cache(maxsize=None)
def lattice(n=len(SITES)):
    return _done(f"lattice({n})", lattice_frame(n, seed=n)[None])


@functools.lru_cache(maxsize=None)
def lattice_movie(seeds=(10, 11, 12, 13)):
    """full lattices that differ in the order of their values, one frame per seed"""
    return _done("lattice_movie", np.stack([lattice_frame(len(SITES), seed=s) for s in seeds]))


@functools.lru_cache(maxsize=None)
def tie_pairs():
    """384 pairs m[y, x] = m[y, x + 1], every pair with a value of its own: both are candidates, the left one is kept"""
    ys, xs = range(1, 47, 3), range(1, 94, 4)
    values = iter(np.random.default_rng(1).permutation(len(ys) * len(xs)) + 1)
    m = np.zeros((H, W), np.float32)
    for y in ys:
        for x in xs:
            m[y, x] = m[y, x + 1] = next(values)
    return _done("tie_pairs", m[None])


@functools.lru_cache(maxsize=None)
def ties_below_a_crowd():
    """336 isolated peaks (rows 0 .. 12 of the lattice) above CROWD; below them 120 tie pairs (rows 16 .. 28) and 92 plateaus
    of 2 x 2 (rows 33 .. 46), each with a value of its own below CROWD: every kept member of a tie has 336 kept before it"""
    rng = np.random.default_rng(2)
    m = np.zeros((H, W), np.float32)
    crowd = SITES[SITES[:, 0] <= 12]
    m[crowd[:, 0], crowd[:, 1]] = CROWD + 1 + rng.permutation(len(crowd))
    pair_at = [(y, x) for y in range(16, 30, 3) for x in range(1, 94, 4)]
    plateau_at = [(y, x) for y in range(33, 46, 4) for x in range(1, 93, 4)]
    values = iter(rng.permutation(len(pair_at) + len(plateau_at)) + 1)
    for y, x in pair_at:
        m[y, x] = m[y, x + 1] = next(values)
    for y, x in plateau_at:
        m[y:y + 2, x:x + 2] = next(values)
    return _done("ties_below_a_crowd", m[None], 1, [("pair", p) for p in pair_at] + [("plateau", p) for p in plateau_at])


# offsets (across, along) from the first pixel of a pair to the second in the strip's own axes: both axes, both diagonals and
# two oblique directions
_AT_3 = [(0, 3), (3, 0), (3, 3), (3, -3), (2, 3), (3, 1)]
_AT_4 = [(0, 4), (4, 0), (4, 4), (4, -4), (1, 4), (4, 2)]


@functools.lru_cache(maxsize=None)
def ties_at_the_spacing():
    """min_distance = 3, two frames.  264 isolated peaks at spacing 4 above CROWD, and in the strip they leave free (frame 0:
    rows 44 .. 47; frame 1: columns 88 .. 95, the same layout transposed) pairs of equal pixels at Chebyshev distance exactly
    3 (both candidates, the one with the higher row-major index dropped) and exactly 4 (both kept), in every direction the
    strip has room for.  pairs: (frame, first pixel, second pixel, distance), first < second in row-major order."""
    rng = np.random.default_rng(3)
    movie = np.zeros((2, H, W), np.float32)
    pairs = []
    for f in range(2):
        ys, xs = (range(0, 44, 4), range(0, 96, 4)) if f == 0 else (range(0, 48, 4), range(0, 88, 4))
        crowd = np.array([(y, x) for y in ys for x in xs])
        movie[f, crowd[:, 0], crowd[:, 1]] = CROWD + 1 + rng.permutation(len(crowd))
        length, width = (W, 4) if f == 0 else (H, 8)                      # the strip: `length` along, `width` across
        offsets = [(d, o) for o3, o4 in zip(_AT_3, _AT_4) for d, o in ((3, o3), (4, o4))]
        offsets = [(d, (a, b)) for d, (a, b) in offsets if abs(a) < width]   # across = first component
        placed, cursor, k = [], 0, 0
        while True:
            d, (across, along) = offsets[k % len(offsets)]
            a0, l0 = 0, cursor - min(along, 0)
            a1, l1 = a0 + across, l0 + along
            if max(l0, l1) >= length:
                break
            placed.append((d, (a0, l0), (a1, l1)))
            cursor = max(l0, l1) + 4                                      # more than min_distance from the next pair
            k += 1
        values = rng.permutation(len(placed)) + 1
        for v, (d, p, q) in zip(values, placed):
            p, q = ((44 + p[0], p[1]), (44 + q[0], q[1])) if f == 0 else ((p[1], 88 + p[0]), (q[1], 88 + q[0]))
            p, q = sorted((p, q))
            assert max(abs(p[0] - q[0]), abs(p[1] - q[1])) == d
            movie[f, p[0], p[1]] = movie[f, q[0], q[1]] = v
            pairs.append((f, p, q, d))
    return _done("ties_at_the_spacing", movie, 3, pairs)


EDGE_COUNTS = (255, 256, "flat", 257, 511, 512, "zero", 513, 1024, 1025, 1152)


@functools.lru_cache(maxsize=None)
def edge_counts():
    """lattice frames of n candidates around the sizes at which tk_select_kernel changes its trip counts, a flat frame
    (constant 7) and an all-zero frame between them"""
    frames = [np.full((H, W), 7.0, np.float32) if n == "flat" else np.zeros((H, W), np.float32) if n == "zero"
              else lattice_frame(n, seed=n) for n in EDGE_COUNTS]
    return _done("edge_counts", np.stack(frames))


def builders():
    return [lattice(), tie_pairs(), ties_below_a_crowd(), ties_at_the_spacing(), edge_counts()]


# ----------------------------------------------------------------------------------------------------------------------
# the restated peak rule in the layout of mivit_dog_peaks
# ----------------------------------------------------------------------------------------------------------------------
def peaks_frame(frame, min_distance, threshold=THRESHOLD, absolute=None):
    """_peaks_numpy of one map -> (coords [n, 2] int64, values [n] float32, n_candidates)"""
    yx, n_cand = T._peaks_numpy(frame, threshold, min_distance, absolute=absolute)
    return yx, frame[yx[:, 0], yx[:, 1]], n_cand


def peaks_ref(maps, min_distance, cap, threshold=THRESHOLD, absolute=None):
    """The outputs of mivit_dog_peaks / mivit_score_peaks for maps [F, H, W] whose frames all fit the capacity -> (want,
    written): zero past count in want, and the masks of what the kernel writes."""
    F = len(maps)
    want = {"count": np.zeros(F, np.int32), "n_candidates": np.zeros(F, np.int32), "coords": np.zeros((F, cap, 2), np.int32),
            "values": np.zeros((F, cap), np.float32)}
    for f in range(F):
        yx, v, n_cand = peaks_frame(maps[f], min_distance, threshold, absolute)
        assert n_cand <= cap
        want["count"][f], want["n_candidates"][f] = len(yx), n_cand
        want["coords"][f, :len(yx)], want["values"][f, :len(yx)] = yx, v
    kept = np.arange(cap)[None, :] < want["count"][:, None]
    return want, {"coords": kept[:, :, None], "values": kept}


# ----------------------------------------------------------------------------------------------------------------------
# stage 2 of the likelihood-ratio detector beyond one wave
# ----------------------------------------------------------------------------------------------------------------------
STAGE2_COUNTS = (63, 64, 65, 127, 128, 129, 304)
STAGE2_SEED, STAGE2_SPOTS = 5, 40
STAGE2_R = 3


def stage2_profile():
    return T.psf_profile(1.0, STAGE2_R)


def stage2_threshold():
    return float(np.float32(T.detection_threshold(1e-2)))


def camera():
    return CAMERA["gain"], CAMERA["offset"], CAMERA["read_var"]


def stage2_sites():
    """the 304 sites ys in 1:48:3, xs in 1:96:5; every other site of the outermost rows and columns is moved onto the frame's
    border (rows 0 and 47, columns 0 and 95), so windows are clipped by one to three pixels on every side"""
    sites = np.array([(y, x) for y in range(1, H, 3) for x in range(1, W, 5)], np.int64)
    k = np.arange(len(sites))
    for axis, lo, hi, last in ((0, 1, 46, H - 1), (1, 1, 91, W - 1)):
        c = sites[:, axis].copy()
        sites[(c == lo) & (k % 2 == 0), axis] = 0
        sites[(c == hi) & (k % 2 == 1), axis] = last
    return sites


Stage2 = namedtuple("Stage2", "movie lists smap")                          # lists: per frame (coords [n, 2] int64, values [n])


@functools.lru_cache(maxsize=None)
def stage2_case():
    movie = camera_movie((len(STAGE2_COUNTS), H, W), seed=STAGE2_SEED, n_spots=STAGE2_SPOTS, **CAMERA)
    movie.setflags(write=False)
    smap = T._score_numpy(movie, stage2_profile(), *camera())
    sites = stage2_sites()
    rng = np.random.default_rng(STAGE2_SEED)
    lists = []
    for f, n in enumerate(STAGE2_COUNTS):
        yx = sites[rng.permutation(len(sites))[:n]]
        lists.append((yx, smap[f, yx[:, 0], yx[:, 1]]))
    return Stage2(movie, tuple(lists), smap)


@functools.lru_cache(maxsize=None)
def stage2_full():
    """one frame (the first of stage2_case) whose list fills the capacity of 2048: the 1152 lattice sites, then repeats"""
    case = stage2_case()
    yx = np.concatenate([SITES, SITES[:2048 - len(SITES)]])
    return Stage2(case.movie[:1], ((yx, case.smap[0, yx[:, 0], yx[:, 1]]),), case.smap[:1])


def stage2_inputs(lists, cap):
    """count_in [F] int32, coords_in [F, cap, 2] int32, values_in [F, cap] float32, zero past the lists"""
    F = len(lists)
    count, coords, values = np.zeros(F, np.int32), np.zeros((F, cap, 2), np.int32), np.zeros((F, cap), np.float32)
    for f, (yx, v) in enumerate(lists):
        count[f] = len(yx)
        coords[f, :len(yx)], values[f, :len(yx)] = yx, v
    return count, coords, values


def with_strays(lists):
    """The lists with a few coordinates replaced by ones outside the frame (negative, == H, == W) in the middle of the second
    chunk of 64 and of the last chunk, where a list is long enough -> (lists as handed to the kernel, lists without them:
    what the kernel has to make of it, in unchanged order)."""
    strays = [(-1, 5), (H, 5), (5, W), (5, -1), (-1, -1), (H, W)]
    given, clean = [], []
    for yx, v in lists:
        yx, v = yx.copy(), v.copy()
        n = len(yx)
        last = (n - 1) // 64 * 64
        at = sorted({p for p in (96, 97, 99, last + (n - last) // 2, last + (n - last) // 2 + 1) if 64 < p < n - 1})
        for k, p in enumerate(at):
            yx[p] = strays[k % len(strays)]
            v[p] = 0.0
        ok = np.ones(n, bool)
        ok[at] = False
        given.append((yx, v))
        clean.append((yx[ok], v[ok]))
    return given, clean


def stage2_ref(movie, lists, cap):
    """restated_stage2 of the lists at capacity cap -> (want dict in the layout of mivit_lrt_peaks, written masks, T of every
    candidate per frame)"""
    count, coords, values = stage2_inputs(lists, cap)
    thr = stage2_threshold()
    kept, kcoords, stats, status, Tall = restated_stage2(movie, stage2_profile(), thr, count, coords, values, *camera())
    w = np.arange(cap)[None, :] < kept[:, None]
    want = {"count": kept, "coords": kcoords, "stats": stats, "status": status}
    ends = np.cumsum(count)
    return want, {"coords": w[:, :, None], "stats": w[:, :, None], "status": w}, np.split(Tall, ends[:-1])


# ----------------------------------------------------------------------------------------------------------------------
# both detectors with their real filters: camera noise without spots
# ----------------------------------------------------------------------------------------------------------------------
# Three frames of 71 x 71: 5 x 2 tiles, the last of each axis 7 wide.  The smallest square whose side is no multiple of 16 and
# that has a frame of more than 256 difference-of-Gaussians candidates: a local maximum of the filtered noise falls on one
# pixel in twenty (219 .. 252 a frame at 66 .. 70, 259 / 247 / 254 here), so nothing smaller gets there.  The score map of a
# 3 x 3 window has one in nine at p_fa = 0.2; at 0.1 it has 389 / 429 / 390 here, inside (256, 512) as well.
NOISE_SHAPE = (3, 71, 71)
NOISE_DOG = dict(sigma1=1.0, sigma2=2.0, threshold_percentage=-1e3, min_distance=1)   # -1000 max lies below every value
NOISE_SCORE_SIGMA, NOISE_SCORE_R, NOISE_SCORE_P_FA = 0.6, 1, 0.1


@functools.lru_cache(maxsize=None)
def noise_movie(shape=NOISE_SHAPE):
    movie = camera_movie(shape, seed=shape[1] * 1000 + shape[2], n_spots=0, **CAMERA)
    movie.setflags(write=False)
    return movie


def noise_score_threshold():
    return float(np.float32(T.detection_threshold(NOISE_SCORE_P_FA)))


def noise_dog_candidates(movie):
    w1, w2 = T.gaussian_half_kernel(NOISE_DOG["sigma1"]), T.gaussian_half_kernel(NOISE_DOG["sigma2"])
    dog = T._dog_numpy(movie, w1, w2)
    return [T._peaks_numpy(d, NOISE_DOG["threshold_percentage"], 1)[1] for d in dog]


def noise_score_candidates(movie):
    smap = T._score_numpy(movie, T.psf_profile(NOISE_SCORE_SIGMA, NOISE_SCORE_R), *camera())
    return [T._peaks_numpy(s, None, 1, absolute=np.float32(noise_score_threshold()))[1] for s in smap]
