"""CPU: the inputs of tests/test_crowded_detection_gpu.py (tests/crowded_common.py) do what they are built for, asserted on
the restatements alone: the candidate and kept counts, that every clash of the tie builders is found against a kept peak of
index 256 or more, that stage 2 keeps and rejects candidates in every chunk of 64, that the noise movies pass 256 candidates,
and that each of six wrong variants of the rules (the ways tk_select_kernel and lr_kernel could be wrong beyond one pass of a
workgroup or one wave) gives another result than the restatement on at least one of these inputs."""
import numpy as np
import pytest

import crowded_common as C
from moleculardiffusion_mivit_amd.helpers import tracking as T


def candidates(frame, min_distance):
    """the candidates of _peaks_numpy, row-major -> (ys, xs)"""
    mask = frame == T._window_max(frame, min_distance)
    if mask.all():
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.nonzero(mask & (frame > np.float32(C.THRESHOLD) * frame.max()))


def clashes(kept, y, x, m):
    return (np.abs(kept[:, 0] - y) <= m) & (np.abs(kept[:, 1] - x) <= m)


def frames_of(case):
    return [(f"{case.name}[{f}]", frame, case.min_distance) for f, frame in enumerate(case.movie)]


def all_frames():
    return [fr for case in C.builders() for fr in frames_of(case)]


# ----------------------------------------------------------------------------------------------------------------------
# counts
# ----------------------------------------------------------------------------------------------------------------------
def test_identity_weights_return_the_map():
    for case in C.builders():
        dog = T._dog_numpy(case.movie, *C.IDENTITY)
        assert dog.dtype == np.float32 and dog.tobytes() == case.movie.tobytes(), case.name


def counts(case):
    return [(n_cand, len(yx)) for yx, _, n_cand in (C.peaks_frame(fr, case.min_distance) for fr in case.movie)]


def test_counts():
    assert len(C.SITES) == 1152
    assert counts(C.lattice()) == [(1152, 1152)]
    assert counts(C.tie_pairs()) == [(768, 384)]
    want = [(0, 0) if isinstance(n, str) else (n, n) for n in C.EDGE_COUNTS]
    assert counts(C.edge_counts()) == want
    assert [n for n, _ in want] == [255, 256, 0, 257, 511, 512, 0, 513, 1024, 1025, 1152]
    flat, zero = C.edge_counts().movie[2], C.edge_counts().movie[6]
    assert flat.min() == flat.max() == 7.0 and not zero.any()


def test_counts_of_the_tie_builders():
    case = C.ties_below_a_crowd()
    frame = case.movie[0]
    crowd = int((frame > C.CROWD).sum())
    pairs = sum(kind == "pair" for kind, _ in case.pairs)
    plateaus = sum(kind == "plateau" for kind, _ in case.pairs)
    assert crowd >= 300 and pairs >= 50 and plateaus >= 10
    assert len(np.unique(frame[frame > C.CROWD])) == crowd                # distinct values
    assert len(np.unique(frame[(frame > 0) & (frame < C.CROWD)])) == pairs + plateaus
    assert counts(case) == [(crowd + 2 * pairs + 4 * plateaus, crowd + pairs + plateaus)] == [(944, 548)]
    case = C.ties_at_the_spacing()
    assert case.min_distance == 3
    for f, (n_cand, n_kept) in enumerate(counts(case)):
        crowd = int((case.movie[f] > C.CROWD).sum())
        at3 = sum(p[0] == f and p[3] == 3 for p in case.pairs)
        at4 = sum(p[0] == f and p[3] == 4 for p in case.pairs)
        assert crowd >= 260 and at3 >= 3 and at4 >= 2
        assert (n_cand, n_kept) == (crowd + 2 * (at3 + at4), crowd + at3 + 2 * at4)
    assert counts(case) == [(292, 281), (278, 274)]
    # the directions: along x, along y, both diagonals, at both distances
    seen = {(d, abs(q[0] - p[0]), q[1] - p[1]) for _, p, q, d in case.pairs}
    for d in (3, 4):
        assert {(d, 0, d), (d, d, 0), (d, d, d)} <= seen
    assert (3, 3, -3) in seen


# ----------------------------------------------------------------------------------------------------------------------
# tie structure
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [C.ties_below_a_crowd, C.ties_at_the_spacing], ids=lambda b: b.__name__)
def test_every_clash_is_with_a_kept_peak_past_the_first_256(build):
    case = build()
    m = case.min_distance
    for frame in case.movie:
        kept = C.peaks_frame(frame, m)[0]
        ys, xs = candidates(frame, m)
        is_kept = {(int(y), int(x)) for y, x in kept}
        dropped = [(int(y), int(x)) for y, x in zip(ys, xs) if (int(y), int(x)) not in is_kept]
        assert len(dropped) == len(ys) - len(kept) >= 3
        for y, x in dropped:
            hit = np.nonzero(clashes(kept, y, x, m))[0]
            assert len(hit) == 1 and hit[0] >= 256, (y, x, hit)
            ky, kx = kept[hit[0]]
            assert frame[ky, kx] == frame[y, x] and (ky, kx) < (y, x)     # an exact tie, lost to the lower index


def test_pairs_at_the_spacing_and_one_past_it():
    case = C.ties_at_the_spacing()
    for f, frame in enumerate(case.movie):
        kept = {(int(y), int(x)) for y, x in C.peaks_frame(frame, 3)[0]}
        for g, p, q, d in case.pairs:
            if g == f:
                assert p in kept and (q in kept) == (d == 4), (f, p, q, d)


# ----------------------------------------------------------------------------------------------------------------------
# stage 2
# ----------------------------------------------------------------------------------------------------------------------
def stage2_keep():
    case = C.stage2_case()
    _, _, Tall = C.stage2_ref(case.movie, case.lists, 304)
    return case, Tall, C.stage2_threshold()


def test_stage2_lists():
    case, Tall, thr = stage2_keep()
    assert tuple(len(yx) for yx, _ in case.lists) == C.STAGE2_COUNTS == (63, 64, 65, 127, 128, 129, 304)
    sites = C.stage2_sites()
    assert len(sites) == len({tuple(s) for s in sites.tolist()}) == 304
    for axis, last in ((0, C.H - 1), (1, C.W - 1)):                       # the border rows and columns are reached
        assert (sites[:, axis] == 0).sum() >= 4 and (sites[:, axis] == last).sum() >= 4
    whole = case.lists[-1][0]
    assert sorted(map(tuple, whole.tolist())) == sorted(map(tuple, sites.tolist()))
    for f, (yx, v) in enumerate(case.lists):
        assert v.dtype == np.float32 and np.array_equal(v, case.smap[f, yx[:, 0], yx[:, 1]])


def test_stage2_keeps_and_rejects_in_every_chunk():
    case, Tall, thr = stage2_keep()
    for Tf in Tall:
        assert not (np.abs(Tf - thr) <= 1e-9 * thr).any()                  # no candidate on the threshold
    keep = Tall[-1] > thr
    for base in range(0, 304, 64):
        k = keep[base:base + 64]
        assert k.any() and not k.all(), base
    for f in (2, 5, 6):                                                    # 65, 129, 304: the last, partial chunk keeps one
        n = len(Tall[f])
        assert n % 64 and (Tall[f][n // 64 * 64:] > thr).any(), f


def test_stage2_full_frame_and_strays():
    full = C.stage2_full()
    yx = full.lists[0][0]
    assert len(yx) == 2048 and np.array_equal(yx[:1152], C.SITES) and np.array_equal(yx[1152:], C.SITES[:896])
    case = C.stage2_case()
    given, clean = C.with_strays(case.lists)
    for f, ((g, _), (c, _)) in enumerate(zip(given, clean)):
        n = C.STAGE2_COUNTS[f]
        out = (g[:, 0] < 0) | (g[:, 0] >= C.H) | (g[:, 1] < 0) | (g[:, 1] >= C.W)
        assert len(g) == n and len(c) == n - out.sum() and not out[:64].any()
        where = np.nonzero(out)[0]
        last = (n - 1) // 64 * 64
        assert ((where > 64) & (where < 127)).any() == (n >= 127)        # in the middle of the second chunk
        assert ((where > last) & (where < n - 1)).any() == (n > 64 and n - last >= 3)   # and of the last one
    strays = np.concatenate([g[(g[:, 0] < 0) | (g[:, 0] >= C.H) | (g[:, 1] < 0) | (g[:, 1] >= C.W)] for g, _ in given])
    assert (strays[:, 0] < 0).any() and (strays[:, 0] == C.H).any() and (strays[:, 1] == C.W).any()


# ----------------------------------------------------------------------------------------------------------------------
# noise movies
# ----------------------------------------------------------------------------------------------------------------------
def test_noise_movie_passes_256_candidates_in_both_detectors():
    movie = C.noise_movie()
    F, H, W = movie.shape
    assert H % 16 and W % 64 and H % 64 and W % 16
    dog = C.noise_dog_candidates(movie)
    score = C.noise_score_candidates(movie)
    assert any(256 < n < 512 for n in dog), dog
    assert any(256 < n < 512 for n in score), score
    assert max(dog) < 512 and max(score) < 512                            # the front ends' default capacity holds them
    assert dog == [259, 247, 254] and score == [389, 429, 390]
    # the threshold of the difference of Gaussians lies below every value
    w1, w2 = T.gaussian_half_kernel(1.0), T.gaussian_half_kernel(2.0)
    d = T._dog_numpy(movie, w1, w2)
    for fr in d:
        assert np.float32(C.NOISE_DOG["threshold_percentage"]) * fr.max() < fr.min()


# ----------------------------------------------------------------------------------------------------------------------
# mutants: the rules, wrong in one way each
# ----------------------------------------------------------------------------------------------------------------------
def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def sort_right(v):
    return np.argsort(-v, kind="stable")


def sort_first_256_only(v):
    return np.concatenate([np.argsort(-v[:256], kind="stable"), np.arange(256, len(v))]) if len(v) > 256 else sort_right(v)


def sort_half_padded(v):
    return np.argsort(-v[:next_pow2(len(v)) // 2], kind="stable")


def sort_ties_by_higher_index(v):
    return np.lexsort((-np.arange(len(v)), -v))


def select(frame, m, order=sort_right, scan=None):
    """the peak rule with its sort and with the part of the kept list that the greedy pass looks at as parameters"""
    ys, xs = candidates(frame, m)
    kept = np.zeros((len(ys), 2), np.int64)
    n = 0
    for i in order(frame[ys, xs]):
        if not clashes(kept[:n if scan is None else min(n, scan)], ys[i], xs[i], m).any():
            kept[n] = ys[i], xs[i]
            n += 1
    return kept[:n]


def test_the_rule_written_here_is_the_restatement():
    for name, frame, m in all_frames():
        assert np.array_equal(select(frame, m), C.peaks_frame(frame, m)[0]), name


PEAK_MUTANTS = {"greedy pass against the first 256 kept only": dict(scan=256),
                "sort of the first 256 keys only": dict(order=sort_first_256_only),
                "sort padded to next_pow2(n) / 2": dict(order=sort_half_padded),
                "ties broken by the higher index": dict(order=sort_ties_by_higher_index)}


@pytest.mark.parametrize("mutant", PEAK_MUTANTS)
def test_peak_mutants_are_told_apart(mutant):
    differs = [name for name, frame, m in all_frames()
               if not np.array_equal(select(frame, m, **PEAK_MUTANTS[mutant]), C.peaks_frame(frame, m)[0])]
    print(mutant, "->", differs)
    assert differs
    if "greedy" in mutant:                                                # only a tie below 256 kept peaks can tell this one
        assert set(differs) == {"tie_pairs[0]", "ties_below_a_crowd[0]", "ties_at_the_spacing[0]", "ties_at_the_spacing[1]"}


def compact_right(yx, keep):
    return yx[keep]


def compact_restarting(yx, keep):
    """the slot of a kept candidate is its rank within its own chunk of 64; the count is still the total"""
    out = np.zeros_like(yx)
    for base in range(0, len(yx), 64):
        k = keep[base:base + 64]
        out[:k.sum()] = yx[base:base + 64][k]
    return out[:keep.sum()]


def compact_first_wave(yx, keep):
    """count_in read as min(count_in, 64)"""
    return yx[:64][keep[:64]]


@pytest.mark.parametrize("mutant", [compact_restarting, compact_first_wave], ids=lambda m: m.__name__)
def test_stage2_mutants_are_told_apart(mutant):
    case, Tall, thr = stage2_keep()
    differs = []
    for f, (yx, _) in enumerate(case.lists):
        keep = Tall[f] > thr
        got, want = mutant(yx, keep), compact_right(yx, keep)
        if len(yx) <= 64:
            assert np.array_equal(got, want)                              # one wave: the mutants are right
        elif not np.array_equal(got, want):
            differs.append(len(yx))
    assert differs == [65, 127, 128, 129, 304]
