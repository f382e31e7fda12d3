"""GPU: particle detection in crowded frames, past one pass of a workgroup and past one wave (csrc/peaks.h, csrc/detect.hip).

Peak selection gets the maps of tests/crowded_common.py through mivit_dog_peaks with identity weights (the difference of
Gaussians is then the movie itself), in guarded, poisoned buffers: 255 .. 1152 candidates per frame, exact ties below more
than 256 kept peaks, capacities that are no power of two and that are filled to the last slot, overflow by hundreds of threads
at once.  Both detectors then run with their real filters on camera noise with more than 256 candidates a frame, and stage 2 of
the likelihood-ratio detector runs on lists of 63 .. 2048 candidates.  tests/test_crowded_detection.py shows on the CPU that
these inputs tell wrong kernels from right ones."""
import functools

import numpy as np
import pytest
import torch

import abi_guard as G
import crowded_common as C
from abi_call import F32, F64, I32, U8, Call, bits_equal, check_all, expect
from lrt_common import CAMERA, restated_stage1
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu


def on_gpu(a):
    return torch.from_numpy(np.array(a)).cuda()                           # a copy: the built inputs are read-only


BUILDERS = {b.__name__: b for b in (C.lattice, C.tie_pairs, C.ties_below_a_crowd, C.ties_at_the_spacing, C.edge_counts)}


# ----------------------------------------------------------------------------------------------------------------------
# peak selection through the raw mivit_dog_peaks
# ----------------------------------------------------------------------------------------------------------------------
def dog_call(movie, min_distance, cap, mis=0, store_dog=1):
    c = Call("mivit_dog_peaks", mis)
    F, H, W = movie.shape
    w1, w2 = C.IDENTITY
    wsb = N.lib.mivit_dog_peaks_workspace_bytes(F, H, W, cap, store_dog)
    ws = c.work(wsb, U8, G.POISON)
    c.run(c.inp("movie", movie, F32), F, H, W, w1.ctypes.data, 0, w2.ctypes.data, 0, C.THRESHOLD, min_distance, cap,
          c.out("count", F, I32), c.out("n_candidates", F, I32), c.out("coords", (F, cap, 2), I32),
          c.out("values", (F, cap), F32), c.out("dog", (F, H, W), F32) if store_dog else None, ws, wsb)
    if store_dog:
        expect(c, "dog", movie)
    return c


@functools.lru_cache(maxsize=None)
def builder_ref(name, cap=2048):
    case = BUILDERS[name]()
    return C.peaks_ref(case.movie, case.min_distance, cap)


def check_frame_fits(c, f, frame, min_distance):
    """frame f of a finished call against the restatement, whatever the other frames of the call did"""
    yx, v, n_cand = C.peaks_frame(frame, min_distance)
    n = len(yx)
    assert c.outs["n_candidates"].numpy()[f] == n_cand and c.outs["count"].numpy()[f] == n, f
    assert np.array_equal(c.outs["coords"].numpy()[f, :n], yx), f
    assert bits_equal(c.outs["values"].numpy()[f, :n], v), f
    assert c.outs["coords"].unchanged()[f, n:].all() and c.outs["values"].unchanged()[f, n:].all(), f


def check_frame_overflows(c, f, frame, min_distance, cap):
    """More candidates than the capacity: which ones were stored is up to the atomics, but the count is reported, every kept
    peak is a candidate with its own value, the kept ones are sorted and spaced, and nothing is written past them."""
    _, _, n_cand = C.peaks_frame(frame, min_distance)
    assert n_cand > cap and c.outs["n_candidates"].numpy()[f] == n_cand
    n = int(c.outs["count"].numpy()[f])
    assert 1 <= n <= cap
    yx, v = c.outs["coords"].numpy()[f, :n].astype(np.int64), c.outs["values"].numpy()[f, :n]
    assert (yx >= 0).all() and (yx[:, 0] < frame.shape[0]).all() and (yx[:, 1] < frame.shape[1]).all()
    assert bits_equal(v, frame[yx[:, 0], yx[:, 1]]) and (v > 0).all()     # non-zero pixels of these maps are the candidates
    assert (np.diff(v) <= 0).all()
    d = np.maximum(np.abs(yx[:, None, 0] - yx[None, :, 0]), np.abs(yx[:, None, 1] - yx[None, :, 1]))
    assert (d[~np.eye(n, dtype=bool)] > min_distance).all()
    assert c.outs["coords"].unchanged()[f, n:].all() and c.outs["values"].unchanged()[f, n:].all()


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("name", BUILDERS)
def test_builders_at_full_capacity(name, mis):
    case = BUILDERS[name]()
    want, written = builder_ref(name)
    assert want["n_candidates"].max() >= 255
    for store_dog in (1, 0):
        c = dog_call(case.movie, case.min_distance, 2048, mis, store_dog)
        check_all(c, want, written)


@pytest.mark.parametrize("cap", [513, 512])
def test_capacities_at_the_count(cap):
    """n2max = 1024 for the capacity 513; at 512 the frame of 512 candidates fills the buffer to its last slot (no overflow)
    and the frame of 513 overflows"""
    edge = C.edge_counts()
    frames = [C.EDGE_COUNTS.index(n) for n in (511, 512, 513)]
    movie = edge.movie[frames]
    for mis, store_dog in ((0, 1), (1, 0)):
        c = dog_call(movie, 1, cap, mis, store_dog)
        for f, n in enumerate((511, 512, 513)):
            if n <= cap:
                check_frame_fits(c, f, movie[f], 1)
            else:
                check_frame_overflows(c, f, movie[f], 1, cap)
    dm = on_gpu(movie)
    if cap == 512:
        with pytest.raises(RuntimeError, match="max_peaks_per_frame"):
            ops.dog_peaks(dm, *C.IDENTITY, C.THRESHOLD, 1, cap, False)
        assert ops.dog_peaks(dm[:2], *C.IDENTITY, C.THRESHOLD, 1, cap, False)[0].tolist() == [511, 512]
    else:
        assert ops.dog_peaks(dm, *C.IDENTITY, C.THRESHOLD, 1, cap, False)[0].tolist() == [511, 512, 513]


def test_a_frame_gives_the_same_bits_wherever_it_stands_and_every_time():
    """the atomics append in any order; the sort alone defines the result"""
    case = C.lattice_movie()
    movie = np.concatenate([case.movie, C.tie_pairs().movie, C.ties_below_a_crowd().movie])
    want, written = C.peaks_ref(movie, 1, 2048)
    first = dog_call(movie, 1, 2048, 0, 0)
    check_all(first, want, written)
    perm = np.array([3, 5, 0, 4, 2, 1])
    for order in (np.arange(len(movie)), perm):
        other = dog_call(movie[order], 1, 2048, 0, 0)
        for name in want:
            assert bits_equal(other.outs[name].numpy(), first.outs[name].numpy()[order]), (name, order)


@pytest.mark.parametrize("cap", [256, 257, 1024])
def test_overflow_in_a_crowd(cap):
    """896, 895 and 128 threads of 18 workgroups a frame find the list full"""
    movie = C.lattice_movie().movie[:2]
    for mis, store_dog in ((0, 0), (1, 1)):
        c = dog_call(movie, 1, cap, mis, store_dog)
        assert c.outs["n_candidates"].numpy().tolist() == [1152, 1152]
        for f in range(2):
            check_frame_overflows(c, f, movie[f], 1, cap)
    with pytest.raises(RuntimeError, match="max_peaks_per_frame"):
        ops.dog_peaks(on_gpu(movie), *C.IDENTITY, C.THRESHOLD, 1, cap, True)


def test_builders_through_ops():
    for name, build in BUILDERS.items():
        case = build()
        want, _ = builder_ref(name)
        count, coords, values, dog = ops.dog_peaks(on_gpu(case.movie), *C.IDENTITY, C.THRESHOLD,
                                                   case.min_distance, max_peaks_per_frame=2048)
        assert np.array_equal(count.cpu().numpy(), want["count"]), name
        assert np.array_equal(coords.cpu().numpy(), want["coords"]), name   # zero past count
        assert bits_equal(values.cpu().numpy(), want["values"]), name
        assert bits_equal(dog.cpu().numpy(), case.movie), name


# ----------------------------------------------------------------------------------------------------------------------
# both detectors with their real filters on camera noise
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise_dog_ref(cap):
    movie = C.noise_movie()
    dog = T._dog_numpy(movie, T.gaussian_half_kernel(1.0), T.gaussian_half_kernel(2.0))
    return C.peaks_ref(dog, 1, cap, threshold=C.NOISE_DOG["threshold_percentage"])[0], dog


@pytest.mark.parametrize("cap", [512, 2048])
def test_dog_peaks_on_noise(cap):
    want, dog = noise_dog_ref(cap)
    assert want["n_candidates"].max() > 256
    dm = on_gpu(C.noise_movie())
    count, coords, values, g_dog = ops.dog_peaks(dm, T.gaussian_half_kernel(1.0), T.gaussian_half_kernel(2.0),
                                                 C.NOISE_DOG["threshold_percentage"], 1, cap, True)
    assert bits_equal(g_dog.cpu().numpy(), dog)
    assert np.array_equal(count.cpu().numpy(), want["count"])
    assert np.array_equal(coords.cpu().numpy(), want["coords"])
    assert bits_equal(values.cpu().numpy(), want["values"])


@pytest.mark.parametrize("cap", [512, 2048])
def test_score_peaks_on_noise(cap):
    movie = C.noise_movie()
    e = T.psf_profile(C.NOISE_SCORE_SIGMA, C.NOISE_SCORE_R)
    thr = C.noise_score_threshold()
    count, coords, values, smap = restated_stage1(movie, e, thr, 1, cap, *C.camera())
    assert count.max() > 256
    g_count, g_coords, g_values, g_map = ops.score_peaks(on_gpu(movie), e, *C.camera(), thr, 1, cap, True)
    assert bits_equal(g_map.cpu().numpy(), smap)
    assert np.array_equal(g_count.cpu().numpy(), count)
    assert np.array_equal(g_coords.cpu().numpy(), coords)
    assert bits_equal(g_values.cpu().numpy(), values)


def test_front_ends_on_noise():
    movie = C.noise_movie()
    dm = on_gpu(movie)
    host, dog_h = T.detect_particles_movie(movie, **C.NOISE_DOG)
    dev, dog_d = T.detect_particles_movie(dm, **C.NOISE_DOG)
    assert max(len(c) for c in host) > 256 and bits_equal(dog_d.cpu().numpy(), dog_h)
    for h, d in zip(host, dev):
        assert d.dtype == h.dtype and np.array_equal(d, h)
    kw = dict(CAMERA, sigma0=C.NOISE_SCORE_SIGMA, radius=C.NOISE_SCORE_R, p_fa=C.NOISE_SCORE_P_FA, min_distance=1)
    host, stats_h, map_h = T.detect_particles_lrt_movie(movie, **kw)
    dev, stats_d, map_d = T.detect_particles_lrt_movie(dm, **kw)
    assert max(len(c) for c in host) > 64 and bits_equal(map_d.cpu().numpy(), map_h)
    for h, d, sh, sd in zip(host, dev, stats_h, stats_d):
        assert d.dtype == h.dtype and np.array_equal(d, h)
        assert np.all(np.abs(sd[:, :3] - sh[:, :3]) <= 1e-9 * np.abs(sh[:, :3]))
        assert bits_equal(sd[:, 3:], sh[:, 3:])                            # the stage-1 statistic and the status


# ----------------------------------------------------------------------------------------------------------------------
# stage 2 beyond one wave
# ----------------------------------------------------------------------------------------------------------------------
def lrt_call(movie, lists, cap, mis=0):
    count, coords, values = C.stage2_inputs(lists, cap)
    e = C.stage2_profile()
    F, H, W = movie.shape
    c = Call("mivit_lrt_peaks", mis)
    c.run(c.inp("movie", movie, F32), F, H, W, e.ctypes.data, C.STAGE2_R, *C.camera(), C.stage2_threshold(), cap,
          c.inp("count_in", count, I32), c.inp("coords_in", coords, I32), c.inp("values_in", values, F32),
          c.out("count", F, I32), c.out("coords", (F, cap, 2), I32), c.out("stats", (F, cap, 4), F64),
          c.out("status", (F, cap), I32))
    return c


def stats_close(got, want, what):
    """T, photons and background within 1e-9 relative (the kernel and the restatement differ by log alone), the stage-1
    statistic bitwise"""
    got, want = got.reshape(-1, 4), want.reshape(-1, 4)
    err = np.abs(got[:, :3] - want[:, :3])
    assert np.all(err <= 1e-9 * np.abs(want[:, :3])), (what, float(err.max()))
    assert bits_equal(got[:, 3], want[:, 3]), what


@functools.lru_cache(maxsize=None)
def stage2(kind, cap):
    """-> (movie, lists handed to the kernel, want, written)"""
    case = C.stage2_full() if kind.startswith("full") else C.stage2_case()
    given, clean = C.with_strays(case.lists) if kind.endswith("strays") else (case.lists, case.lists)
    want, written, _ = C.stage2_ref(case.movie, clean, cap)
    return case.movie, given, want, written


STAGE2 = [("case", 304), ("case", 2048), ("case-strays", 304), ("case-strays", 2048), ("full", 2048), ("full-strays", 2048)]


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("kind,cap", STAGE2, ids=[f"{k}-cap{c}" for k, c in STAGE2])
def test_stage2_beyond_one_wave(kind, cap, mis):
    movie, lists, want, written = stage2(kind, cap)
    assert want["count"].min() >= 1 and max(len(yx) for yx, _ in lists) == (2048 if kind.startswith("full") else 304)
    if kind.endswith("strays"):
        plain = stage2(kind.split("-")[0], cap)[2]
        assert (want["count"] <= plain["count"]).all()
    c = lrt_call(movie, lists, cap, mis)
    check_all(c, want, written, close={"stats": stats_close})


@pytest.mark.parametrize("cap", [304, 2048])
def test_stage2_through_ops_and_frame_by_frame(cap):
    movie, lists, want, _ = stage2("case-strays", cap)
    dm = on_gpu(movie)
    e = C.stage2_profile()
    count, coords, values = (on_gpu(a) for a in C.stage2_inputs(lists, cap))

    def run(sl):
        return [t.cpu().numpy() for t in ops.lrt_peaks(dm[sl].clone(), e, *C.camera(), C.stage2_threshold(), count[sl].clone(),
                                                       coords[sl].clone(), values[sl].clone())]

    whole = run(slice(None))
    assert np.array_equal(whole[0], want["count"])
    assert np.array_equal(whole[1], want["coords"])                       # in stage-1 order, zero past count
    assert np.array_equal(whole[3], want["status"])
    stats_close(whole[2], want["stats"], "ops.lrt_peaks")
    for f in range(len(movie)):
        alone = run(slice(f, f + 1))
        for a, w in zip(alone, whole):
            assert bits_equal(a[0], w[f]), f
