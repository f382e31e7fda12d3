"""GPU: the linking kernels (csrc/linking.hip, ops.link_frames / ops.chain_tracks) against their numpy restatement
(helpers/tracking.py) on every pair of the fixture tests/golden/tracking_link/link.npz, against scipy on the pairs whose
optimum is unique, and the whole track_particles_flat(linking="device") against the host path.  Equality everywhere: kernel
and restatement are one algorithm in one order of operations.  Fixed inputs, every launch runs once (twice for the
determinism check)."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import linking_common as lc
import tracking_common as tc
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return lc.load()


def _quiet(fn, *a, **kw):
    with redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _device(frames, cap=None):
    padded, counts = T._padded_detections(frames, None)
    if cap is not None and cap > padded.shape[1]:
        padded = np.concatenate([padded, np.zeros((len(padded), cap - padded.shape[1], 2), np.int32)], axis=1)
    return padded, counts, torch.from_numpy(padded).cuda(), torch.from_numpy(counts).cuda()


def test_kernel_equals_the_restatement_on_every_pair_and_is_deterministic(fixture):
    """All cases of the fixture concatenated along F with movie_start: one launch, ties included."""
    frames, starts = [], []
    for name, (fr, _, _) in fixture.items():
        if name == "full_512":
            continue                                                     # its own test below
        frames += fr
        starts += [1] + [0] * (len(fr) - 1)
    padded, counts, dcoords, dcount = _device(frames)
    want = T.link_particles_movie(padded, counts, lc.MAX_DISTANCE, movie_start=starts)
    got = ops.link_frames(dcoords, dcount, lc.MAX_DISTANCE, movie_start=torch.tensor(starts, device="cuda"))
    again = ops.link_frames(dcoords, dcount, lc.MAX_DISTANCE, movie_start=starts)
    assert got.dtype == torch.int32 and got.shape == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, again)
    # before the max_distance filter too
    want_all = T.link_particles_movie(padded, counts, float("inf"), movie_start=starts)
    got_all = ops.link_frames(dcoords, dcount, float("inf"), movie_start=starts)
    assert np.array_equal(got_all.cpu().numpy(), want_all)
    # through the public entry point
    assert torch.equal(T.link_particles_movie(dcoords, dcount, lc.MAX_DISTANCE, movie_start=starts), got)


def test_kernel_equals_scipy_where_the_optimum_is_unique(fixture):
    checked = 0
    for name, (frames, links, flags) in fixture.items():
        if name == "full_512":
            continue
        _, _, dcoords, dcount = _device(frames)
        got = ops.link_frames(dcoords, dcount, lc.MAX_DISTANCE).cpu().numpy()
        for p in range(len(frames) - 1):
            if not flags[p]:
                continue
            scipy_links, _, _ = T.link_particles(frames[p], frames[p + 1], lc.MAX_DISTANCE)
            assert lc.link_set(got[p + 1], len(frames[p + 1])) == set(scipy_links) == links[p], (name, p)
            checked += 1
    assert checked > 850


HAND_COUNTS = np.array([2, 3, 1, 2], np.int32)
HAND_LINK = np.array([[-1, -1, -1, -1], [1, -1, 0, -1], [1, -1, -1, -1], [-1, 0, -1, -1]], np.int32)


def test_chain_kernel_on_hand_written_links_and_against_the_restatement():
    link, count = torch.from_numpy(HAND_LINK).cuda(), torch.from_numpy(HAND_COUNTS).cuda()
    for ms in (None, [1, 0, 1, 0]):
        ids, lengths, n = ops.chain_tracks(link, count, movie_start=ms)
        wids, wlen, wn = T.chain_tracks(HAND_LINK, HAND_COUNTS, movie_start=ms)
        assert np.array_equal(ids.cpu().numpy(), wids) and np.array_equal(lengths.cpu().numpy(), wlen) and int(n) == int(wn[0])
    ids, lengths, n = ops.chain_tracks(link, count)
    assert ids.cpu().tolist() == [[0, 1, -1, -1], [1, 2, 0, -1], [2, -1, -1, -1], [3, 2, -1, -1]]
    assert lengths[:4].cpu().tolist() == [2, 2, 3, 1] and int(n) == 4
    # more than 256 detections per frame (several scan chunks), empty frames, no frames
    rng = np.random.default_rng(8)
    F, cap = 7, 700
    counts = np.array([700, 650, 0, 300, 257, 256, 1], np.int32)
    big = np.full((F, cap), -1, np.int32)
    for f in range(1, F):
        m = min(counts[f], counts[f - 1])
        partners = rng.permutation(counts[f - 1])[:m]
        slots = rng.permutation(counts[f])[:m]
        keep = rng.random(m) < 0.7
        big[f, slots[keep]] = partners[keep]
    ids, lengths, n = ops.chain_tracks(torch.from_numpy(big).cuda(), torch.from_numpy(counts).cuda())
    wids, wlen, wn = T.chain_tracks(big, counts)
    assert np.array_equal(ids.cpu().numpy(), wids) and np.array_equal(lengths.cpu().numpy(), wlen) and int(n) == int(wn[0])
    ids, lengths, n = ops.chain_tracks(torch.zeros(0, 4, dtype=torch.int32, device="cuda"),
                                       torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert ids.shape == (0, 4) and int(n) == 0


@pytest.mark.parametrize("name", list(tc.MOVIES))
def test_chain_and_table_reproduce_the_host_book_keeping(name):
    coords, _ = T.detect_particles_movie(tc.movie(name))
    want_tracks, want_det, want_n = T._link_tracks(coords, 15, 5)
    padded, counts, dcoords, dcount = _device(coords)
    link = ops.link_frames(dcoords, dcount, 15)
    ids, lengths, n = ops.chain_tracks(link, dcount)
    assert int(n) == want_n
    fr, y, x, tid, in_long = (a.cpu().numpy() for a in T._detections_table(dcoords, dcount, ids, lengths, 5))
    for col, got in zip(("frame", "y", "x", "track_id"), (fr, y, x, tid)):
        assert np.array_equal(got, want_det[col]), col
    assert T._tracks_from_table(fr, y, x, tid, in_long) == want_tracks


@pytest.mark.parametrize("name", list(tc.MOVIES))
def test_whole_movie_device_linking_equals_host_linking(name):
    mov = torch.from_numpy(tc.movie(name)).cuda()
    tracks, det, dog = _quiet(T.track_particles_flat, mov, min_track_length=5, linking="device")
    host_tracks, host_det, host_dog = _quiet(T.track_particles_flat, mov, min_track_length=5, linking="host")
    assert tracks == host_tracks and list(tracks) == list(host_tracks)
    assert list(det) == list(host_det)
    for col in det:
        assert det[col].dtype == np.int64 and np.array_equal(det[col], host_det[col]), col
    assert dog.is_cuda and torch.equal(dog, host_dog)
    gold = np.load(tc.GOLDEN)
    rows = np.array([(tid, fr, y, x) for tid, pos in tracks.items() for fr, y, x in pos], np.int64)
    assert np.array_equal(rows, gold[f"{name}_tracks"])
    # the tensors variant feeds the patch gather and the fit without leaving the device
    t, _ = T.track_particles_tensors(mov, min_track_length=5)
    keep = t["in_long_track"]
    assert t["frame"].is_cuda and np.array_equal(t["track_id"].cpu().numpy(), det["track_id"])
    patches = T.extract_patches_flat(mov, t["frame"][keep], t["y"][keep], t["x"][keep], tc.PATCH_SIZE)
    k = keep.cpu().numpy()
    want = T.extract_patches_flat(mov, det["frame"][k], det["y"][k], det["x"][k], tc.PATCH_SIZE)
    assert patches.is_cuda and torch.equal(patches, want)
    res = T.refine_localizations(patches, t["y"][keep], t["x"][keep])
    ref = T.refine_localizations(want, det["y"][k], det["x"][k])
    assert np.array_equal(res["x_refined"], ref["x_refined"])


def test_concatenated_movies_equal_the_movies_one_by_one():
    movies = [torch.from_numpy(tc.movie(n)[:, :97, :128]).cuda() for n in ("main", "odd")]
    both = torch.cat(movies)
    starts = torch.zeros(len(both), dtype=torch.bool, device="cuda")
    starts[0] = starts[len(movies[0])] = True
    t, _ = T.track_particles_tensors(both, min_track_length=1, movie_start=starts)
    off_frame, off_id, at = 0, 0, 0
    for mov in movies:
        one, _ = T.track_particles_tensors(mov, min_track_length=1)
        n = len(one["frame"])
        assert torch.equal(t["frame"][at:at + n], one["frame"] + off_frame)
        assert torch.equal(t["y"][at:at + n], one["y"]) and torch.equal(t["x"][at:at + n], one["x"])
        assert torch.equal(t["track_id"][at:at + n], one["track_id"] + off_id)
        off_frame, off_id, at = off_frame + len(mov), off_id + int(one["n_tracks"]), at + n
    assert at == len(t["frame"]) and int(t["n_tracks"]) == off_id


def test_full_512_pair_and_the_limit(fixture):
    frames, links, flags = fixture["full_512"]
    padded, counts, dcoords, dcount = _device(frames, cap=512)
    assert dcoords.shape == (2, 512, 2)
    got = ops.link_frames(dcoords, dcount, lc.MAX_DISTANCE).cpu().numpy()
    assert np.array_equal(got, T.link_particles_movie(padded, counts, lc.MAX_DISTANCE))
    got_all = ops.link_frames(dcoords, dcount, float("inf")).cpu().numpy()
    assert np.array_equal(got_all, T.link_particles_movie(padded, counts, float("inf")))
    assert sorted(got_all[1].tolist()) == list(range(512))
    if flags[0]:
        assert lc.link_set(got[1], 512) == links[0]
    # the limit: checked before any launch, named in the message
    cap = ops.LINK_MAX_DETECTIONS + 1
    too_many = torch.zeros(2, cap, 2, dtype=torch.int32, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="LINK_MAX_DETECTIONS"):
        ops.link_frames(too_many, n)
    with pytest.raises(ValueError, match="LINK_MAX_DETECTIONS"):
        ops.chain_tracks(torch.zeros(2, cap, dtype=torch.int32, device="cuda"), n)
    with pytest.raises(ValueError, match="LINK_MAX_DETECTIONS"):
        T.link_particles_movie(too_many, n)
    with pytest.raises(ValueError, match="LINK_MAX_DETECTIONS"):
        T.track_particles_tensors(torch.zeros(2, 40, 40, device="cuda"), max_peaks_per_frame=cap)
    # at the limit it runs
    full = torch.zeros(2, ops.LINK_MAX_DETECTIONS, 2, dtype=torch.int32, device="cuda")
    full[:, :, 1] = torch.arange(ops.LINK_MAX_DETECTIONS, device="cuda") * 3
    n[:] = 40
    assert ops.link_frames(full, n)[1, :40].cpu().tolist() == list(range(40))


def test_argument_errors_and_empty_input():
    c = torch.zeros(3, 4, 2, dtype=torch.int32, device="cuda")
    n = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert (ops.link_frames(c, n) == -1).all()                                  # empty frames
    assert ops.link_frames(c[:0], n[:0]).shape == (0, 4)                       # F = 0
    assert (ops.link_frames(c[:1], n[:1] + 2) == -1).all()                     # F = 1
    with pytest.raises(ValueError, match="int32 GPU tensor"):
        ops.link_frames(c.cpu(), n)
    with pytest.raises(ValueError, match="int32 GPU tensor"):
        ops.link_frames(c.long(), n)
    with pytest.raises(ValueError, match="count must be"):
        ops.link_frames(c, n[:2])
    with pytest.raises(ValueError, match="one entry per frame"):
        ops.link_frames(c, n, movie_start=[1, 0])
    with pytest.raises(ValueError, match="NaN"):
        ops.link_frames(c, n, float("nan"))
    with pytest.raises(ValueError, match="int32 GPU tensor"):
        ops.chain_tracks(torch.zeros(3, 4, device="cuda"), n)
