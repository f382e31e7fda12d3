"""GPU: the likelihood-ratio detector of csrc/detect.hip against its restatements (helpers/tracking._score_numpy, the numpy
peak rule, _lrt_numpy): the score map and the stage-1 candidates bitwise, stage 2 to the rounding of log, batch independence,
the capacity overflow inside guarded buffers, and the detector through the tracking pipeline."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_guard as G
from abi_call import F32, F64, I32, U8, Call, bits_equal
from lrt_common import CAMERA, camera_movie, restated_stage1, restated_stage2, spot_image
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as GEN
from moleculardiffusion_mivit_amd.helpers import models as M
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

SIGMA = {1: 0.6, 3: 1.0, 7: 2.2}                                          # a width that fills a window of each radius
MIN_DISTANCE, CAP = 3, 64
# frames of 8 x 8 are the smallest that r = 7 allows; 17 x 65 is one past a 16 x 64 tile on both axes, 33 x 130 two past two
# tiles on x; 64 x 64 ends on tile edges.  (shape, radii, flat frame, zero frame)
MOVIES = [((1, 8, 8), (7,), None, None), ((3, 17, 65), (1, 3, 7), 1, None), ((5, 33, 130), (1, 3, 7), 1, 3),
          ((2, 64, 64), (1, 3, 7), None, None)]
CASES = [(shape, r, flat, zero) for shape, radii, flat, zero in MOVIES for r in radii]
IDS = [f"{'x'.join(map(str, c[0]))}-r{c[1]}" for c in CASES]


def _movie(shape, flat, zero):
    return camera_movie(shape, seed=shape[1] * 1000 + shape[2], n_spots=2 if shape[1] == 8 else 4, flat=flat, zero=zero,
                        **CAMERA)


def _cam():
    return CAMERA["gain"], CAMERA["offset"], CAMERA["read_var"]


@pytest.mark.parametrize("shape,r,flat,zero", CASES, ids=IDS)
def test_score_map_and_candidates_bitwise(shape, r, flat, zero):
    movie = _movie(shape, flat, zero)
    e = T.psf_profile(SIGMA[r], r)
    thr = float(np.float32(T.detection_threshold(1e-4)))
    count, coords, values, smap = restated_stage1(movie, e, thr, MIN_DISTANCE, CAP, *_cam())
    assert count.sum() >= 1 and np.isfinite(smap).all()
    if flat is not None:
        assert count[flat] == 0
    if zero is not None:
        assert count[zero] == 0
    dm = torch.from_numpy(movie).cuda()
    for return_map in (True, False):
        g_count, g_coords, g_values, g_map = ops.score_peaks(dm, e, *_cam(), thr, MIN_DISTANCE, CAP, return_map)
        assert np.array_equal(g_count.cpu().numpy(), count)
        assert np.array_equal(g_coords.cpu().numpy(), coords)
        assert bits_equal(g_values.cpu().numpy(), values)
        if return_map:
            assert g_map.dtype == torch.float32 and bits_equal(g_map.cpu().numpy(), smap)
        else:
            assert g_map is None


STAGE2 = [((3, 17, 65), 3, 1, None), ((5, 33, 130), 3, 1, 3), ((2, 64, 64), 1, None, None), ((2, 64, 64), 7, None, None),
          ((1, 8, 8), 7, None, None)]


@pytest.mark.parametrize("shape,r,flat,zero", STAGE2, ids=[f"{'x'.join(map(str, c[0]))}-r{c[1]}" for c in STAGE2])
def test_likelihood_ratio_at_the_candidates(shape, r, flat, zero):
    movie = _movie(shape, flat, zero)
    e = T.psf_profile(SIGMA[r], r)
    thr = float(np.float32(T.detection_threshold(1e-2)))                  # loose: noise candidates that stage 2 has to judge
    count, coords, values, _ = restated_stage1(movie, e, thr, MIN_DISTANCE, CAP, *_cam())
    kept, kcoords, stats, status, Tall = restated_stage2(movie, e, thr, count, coords, values, *_cam())
    assert count.sum() >= 1 and kept.sum() >= 1
    assert not (np.abs(Tall - thr) <= 1e-9 * thr).any()                    # the precondition: no candidate sits on the threshold
    dev = "cuda"
    g_kept, g_coords, g_stats, g_status = ops.lrt_peaks(torch.from_numpy(movie).to(dev), e, *_cam(), thr,
                                                        torch.from_numpy(count).to(dev), torch.from_numpy(coords).to(dev),
                                                        torch.from_numpy(values).to(dev))
    assert g_stats.dtype == torch.float64 and g_stats.shape == (shape[0], CAP, 4) and g_status.dtype == torch.int32
    assert np.array_equal(g_kept.cpu().numpy(), kept)
    assert np.array_equal(g_coords.cpu().numpy(), kcoords)                 # the kept list, in stage-1 order, zero past it
    assert np.array_equal(g_status.cpu().numpy(), status)
    got = g_stats.cpu().numpy()
    for k, name in enumerate(("T", "photons", "background")):
        err = np.abs(got[:, :, k] - stats[:, :, k])
        assert np.all(err <= 1e-9 * np.abs(stats[:, :, k])), (name, float(err.max()))
    assert bits_equal(got[:, :, 3], stats[:, :, 3])                        # the stage-1 statistic is handed through


SPOTS = [(8, 8, 2000.0), (5, 30, 500.0), (2, 50, 1000.0), (12, 60, 300.0)]


@pytest.mark.parametrize("kind", ["cap", "unfactorable"])
def test_stage2_at_the_iteration_cap_and_with_a_matrix_that_never_factors(kind):
    """The two exits of the damped loop that no candidate of the movies above takes, on one 16 x 64 frame with the candidates
    given.  "cap": Poisson spots on no background and no read noise; the outer pixels of a window hold 0 photons, the deviance
    falls all the way to the edge of the domain (mu = 0 there), every step across it is refused and the undamped step never
    gets small: status 2 where the draw puts the optimum on the edge.  "unfactorable": a gain of 1e298 turns the frame into
    photons of 1e-304, the matrix entries sum 1 / mu pass 1e300, no damping makes the matrix factor and 14 failed
    factorisations take lambda past 1e10: status 1, with the start as the answer."""
    r = 3
    e = T.psf_profile(SIGMA[r], r)
    rng = np.random.default_rng(5)
    if kind == "cap":
        movie, cam = rng.poisson(spot_image(16, 64, SPOTS, 0.0)).astype(np.float32)[None], (1.0, 0.0, 0.0)
    else:
        movie, cam = (rng.poisson(spot_image(16, 64, SPOTS, 5.0)) * 1e-6).astype(np.float32)[None], (1e298, 0.0, 0.0)
    count = np.array([len(SPOTS)], np.int32)
    coords = np.zeros((1, CAP, 2), np.int32)
    coords[0, :len(SPOTS)] = [s[:2] for s in SPOTS]
    values = np.zeros((1, CAP), np.float32)
    kept, kcoords, stats, status, _ = restated_stage2(movie, e, 0.0, count, coords, values, *cam)
    assert kept[0] == len(SPOTS)
    assert (status[0, :4] == 2).sum() >= 2 if kind == "cap" else (status[0, :4] == 1).all()
    dev = "cuda"
    g_kept, g_coords, g_stats, g_status = ops.lrt_peaks(torch.from_numpy(movie).to(dev), e, *cam, 0.0, torch.from_numpy(count).to(dev),
                                                        torch.from_numpy(coords).to(dev), torch.from_numpy(values).to(dev))
    assert np.array_equal(g_kept.cpu().numpy(), kept) and np.array_equal(g_coords.cpu().numpy(), kcoords)
    assert np.array_equal(g_status.cpu().numpy(), status)
    got = g_stats.cpu().numpy()
    for k, name in enumerate(("T", "photons", "background")):
        err = np.abs(got[:, :, k] - stats[:, :, k])
        print(f"{kind} {name}: worst relative difference {float(np.nanmax(err[0, :4] / np.abs(stats[0, :4, k])))}")
        assert np.all(err <= 1e-9 * np.abs(stats[:, :, k])), (name, float(err.max()))


def test_stage2_rejects_some_candidates():
    """the two stages differ: over the movies of this file, some stage-1 candidates fail the likelihood ratio"""
    shape, r, flat, zero = STAGE2[1]
    movie = _movie(shape, flat, zero)
    e = T.psf_profile(SIGMA[r], r)
    thr = float(np.float32(T.detection_threshold(1e-2)))
    count, coords, values, _ = restated_stage1(movie, e, thr, MIN_DISTANCE, CAP, *_cam())
    dm = torch.from_numpy(movie).cuda()
    g_count, g_coords, g_values, _ = ops.score_peaks(dm, e, *_cam(), thr, MIN_DISTANCE, CAP, False)
    g_kept = ops.lrt_peaks(dm, e, *_cam(), thr, g_count, g_coords, g_values)[0]
    assert 0 < int(g_kept.sum()) < int(count.sum())


def test_batch_independence():
    shape, r = (5, 33, 130), 3
    movie = _movie(shape, 1, 3)
    e = T.psf_profile(SIGMA[r], r)
    thr = float(np.float32(T.detection_threshold(1e-2)))
    dm = torch.from_numpy(movie).cuda()

    def run(m):
        count, coords, values, smap = ops.score_peaks(m, e, *_cam(), thr, MIN_DISTANCE, CAP, True)
        return [t.cpu().numpy() for t in (smap, count, coords, values) + ops.lrt_peaks(m, e, *_cam(), thr, count, coords, values)]

    whole = run(dm)
    assert whole[4].sum() >= 3
    for f in range(shape[0]):
        alone = run(dm[f:f + 1].clone())
        for a, w in zip(alone, whole):
            assert bits_equal(a[0], w[f])


# ----------------------------------------------------------------------------------------------------------------------
# overflow, inside guarded buffers
# ----------------------------------------------------------------------------------------------------------------------
def _three_spots():
    img = spot_image(32, 32, [(8, 8, 2000.0), (8, 24, 1500.0), (24, 16, 1000.0)], 5.0)
    return (np.random.default_rng(1).poisson(img) * CAMERA["gain"] + CAMERA["offset"]).astype(np.float32)[None]


def test_overflow_raises_naming_the_argument():
    dm = torch.from_numpy(_three_spots()).cuda()
    e = T.psf_profile(1.0, 3)
    for return_map in (True, False):
        with pytest.raises(RuntimeError, match="max_peaks_per_frame"):
            ops.score_peaks(dm, e, *_cam(), 22.0, MIN_DISTANCE, 2, return_map)
        with pytest.raises(RuntimeError, match="max_peaks_per_frame"):
            T.detect_particles_lrt_movie(dm, **CAMERA, max_peaks_per_frame=2, return_map=return_map)
    assert ops.score_peaks(dm, e, *_cam(), 22.0, MIN_DISTANCE, 3, False)[0].tolist() == [3]


@pytest.mark.parametrize("store_map", [1, 0], ids=["map returned", "map in the workspace"])
def test_overflow_stays_inside(store_map):
    movie = _three_spots()
    e = T.psf_profile(1.0, 3)
    F_, H, W, cap = 1, 32, 32, 2
    c = Call("mivit_score_peaks")
    wsb = N.lib.mivit_score_peaks_workspace_bytes(F_, H, W, cap, store_map)
    ws = c.work(wsb, U8, G.POISON)
    c.run(c.inp("movie", movie, F32), F_, H, W, e.ctypes.data, 3, *_cam(), 22.0, MIN_DISTANCE, cap, c.out("count", F_, I32),
          c.out("n_candidates", F_, I32), c.out("coords", (F_, cap, 2), I32), c.out("values", (F_, cap), F32),
          c.out("map", (F_, H, W), F32) if store_map else None, ws, wsb)
    assert c.outs["n_candidates"].numpy().tolist() == [3]
    count = int(c.outs["count"].numpy()[0])
    assert 1 <= count <= 2
    assert c.outs["coords"].untouched(np.arange(cap)[None, :, None].repeat(2, 2) >= count)
    assert c.outs["values"].untouched(np.arange(cap)[None, :] >= count)
    if store_map:
        assert bits_equal(c.outs["map"].numpy(), T._score_numpy(movie, e, *_cam()))
    # stage 2 on a candidate list that claims more entries than the capacity: read as the capacity, nothing written past it
    smap = T._score_numpy(movie, e, *_cam())
    cand = np.array([[[8, 8], [8, 24]]], np.int32)
    vals = smap[0, cand[0, :, 0], cand[0, :, 1]][None]
    d = Call("mivit_lrt_peaks")
    d.run(d.inp("movie", movie, F32), F_, H, W, e.ctypes.data, 3, *_cam(), 1e9, cap, d.inp("count_in", np.array([5]), I32),
          d.inp("coords_in", cand, I32), d.inp("values_in", vals, F32), d.out("count", F_, I32), d.out("coords", (F_, cap, 2), I32),
          d.out("stats", (F_, cap, 4), F64), d.out("status", (F_, cap), I32))
    assert d.outs["count"].numpy().tolist() == [0]                        # nothing passes a threshold of 1e9
    assert d.outs["coords"].untouched() and d.outs["stats"].untouched() and d.outs["status"].untouched()
    d = Call("mivit_lrt_peaks")
    d.run(d.inp("movie", movie, F32), F_, H, W, e.ctypes.data, 3, *_cam(), 22.0, cap, d.inp("count_in", np.array([5]), I32),
          d.inp("coords_in", cand, I32), d.inp("values_in", vals, F32), d.out("count", F_, I32), d.out("coords", (F_, cap, 2), I32),
          d.out("stats", (F_, cap, 4), F64), d.out("status", (F_, cap), I32))
    assert d.outs["count"].numpy().tolist() == [2] and np.array_equal(d.outs["coords"].numpy(), cand)
    assert bits_equal(d.outs["stats"].numpy()[0, :, 3], vals[0].astype(np.float64))


def test_c_abi_rejects_bad_arguments_before_any_launch():
    e = T.psf_profile(1.0, 3)
    fake = 0x1000                                                          # never dereferenced
    ok = dict(F=1, H=16, W=16, r=3, gain=1.0, offset=0.0, read_var=0.0, thr=9.0, md=3, cap=8)
    for change, word in ((dict(r=0), "radius"), (dict(r=8), "radius"), (dict(H=3), "radius"), (dict(gain=0.0), "gain"),
                         (dict(read_var=-1.0), "read_var"), (dict(offset=float("nan")), "offset"), (dict(md=0), "min_distance"),
                         (dict(md=17), "min_distance"), (dict(cap=0), "capacity"), (dict(cap=2049), "capacity"),
                         (dict(thr=float("nan")), "threshold"), (dict(thr=-1.0), "threshold")):
        a = {**ok, **change}
        rc = N.lib.mivit_score_peaks(fake, a["F"], a["H"], a["W"], e.ctypes.data, a["r"], a["gain"], a["offset"], a["read_var"],
                                     a["thr"], a["md"], a["cap"], fake, fake, fake, fake, None, fake, 1 << 30, None)
        assert rc != 0 and word in N.last_error(), (change, N.last_error())
        if "md" not in change:
            rc = N.lib.mivit_lrt_peaks(fake, a["F"], a["H"], a["W"], e.ctypes.data, a["r"], a["gain"], a["offset"], a["read_var"],
                                       a["thr"], a["cap"], fake, fake, fake, fake + 64, fake + 64, fake, fake, None)
            assert rc != 0 and word in N.last_error(), (change, N.last_error())
    bad = e.copy()
    bad[2] = 0.0
    rc = N.lib.mivit_score_peaks(fake, 1, 16, 16, bad.ctypes.data, 3, 1.0, 0.0, 0.0, 9.0, 3, 8, fake, fake, fake, fake, None, fake,
                                 1 << 30, None)
    assert rc != 0 and "profile" in N.last_error()
    rc = N.lib.mivit_score_peaks(fake, 1, 16, 16, e.ctypes.data, 3, 1.0, 0.0, 0.0, 9.0, 3, 8, fake, fake, fake, fake, None, fake, 8,
                                 None)
    assert rc != 0 and "workspace" in N.last_error()
    dm = torch.zeros(1, 16, 16, device="cuda")
    for kw, word in ((dict(gain=0.0), "gain"), (dict(read_var=-1.0), "read_var"), (dict(threshold=-1.0), "threshold"),
                     (dict(min_distance=0), "min_distance"), (dict(max_peaks_per_frame=4096), "max_peaks_per_frame")):
        with pytest.raises(ValueError, match=word):
            ops.score_peaks(dm, e, **kw)
    with pytest.raises(ValueError, match="profile"):
        ops.score_peaks(dm, np.ones(17))
    with pytest.raises(ValueError, match="finite"):
        T.detect_particles_lrt_movie(torch.full((1, 16, 16), float("nan"), device="cuda"))


# ----------------------------------------------------------------------------------------------------------------------
# through the pipeline
# ----------------------------------------------------------------------------------------------------------------------
SIM_CAMERA = {"background": 10.0, "gain": 2.0, "offset": 100.0, "read_noise": 2.0}


def _sim():
    movie, _ = GEN.simulate_movie(4, 12, 64, 64, 0.3, 4, image_props={"particle_intensity": [300.0, 5.0]}, camera=SIM_CAMERA,
                                  generator=torch.Generator().manual_seed(6))
    props = dict(GEN.DEFAULT_IMAGE_PROPS)
    det = {"method": "lrt", "gain": SIM_CAMERA["gain"], "offset": SIM_CAMERA["offset"],
           "read_var": (SIM_CAMERA["read_noise"] / SIM_CAMERA["gain"]) ** 2,
           "sigma0": GEN.psf_sigma_hr(props) / props["upsampling_factor"], "p_fa": 1e-6}
    return movie, det


def test_detector_through_the_pipeline():
    movie, det = _sim()
    dm = movie.cuda()
    tracks_h, table_h, map_h = T.track_particles_flat(movie.numpy(), linking="device", detector=det)
    assert len(tracks_h) >= 3 and len(table_h["frame"]) >= 30
    table_g, map_g = T.track_particles_tensors(dm, detector=det)
    for k in ("frame", "y", "x", "track_id"):
        assert np.array_equal(table_g[k].cpu().numpy(), table_h[k]), k
    assert bits_equal(map_g.cpu().numpy(), map_h)
    tracks_g, table_f, map_f = T.track_particles_flat(dm, linking="device", detector=det)
    assert tracks_g == tracks_h and bits_equal(map_f.cpu().numpy(), map_h)
    # both stages by hand give the detections of the table
    coords, stats, _ = T.detect_particles_lrt_movie(dm, **{k: v for k, v in det.items() if k != "method"})
    assert sum(len(c) for c in coords) == len(table_h["frame"])
    assert all(s.shape == (len(c), 5) for c, s in zip(coords, stats))
    # max_gap and the host loop take the detector too
    gap = T.track_particles_tensors(dm, detector=det, max_gap=2, return_dog=False)
    assert "filled" in gap[0] and gap[1] is None
    assert T.track_particles_flat(dm, linking="host", detector=det)[0].keys() == T.track_particles_flat(
        movie.numpy(), linking="host", detector=det)[0].keys()
    with pytest.raises(ValueError, match="keys"):
        T.track_particles_tensors(dm, detector={"method": "lrt", "threshold": 3.0})
    with pytest.raises(ValueError, match="method"):
        T.track_particles_tensors(dm, detector={"method": "dog"})


def test_detector_none_is_the_path_of_before():
    movie, _ = _sim()
    dm = movie.cuda()
    table, dog = T.track_particles_tensors(dm, detector=None)
    table0, dog0 = T.track_particles_tensors(dm)
    w1, w2 = T.gaussian_half_kernel(1.0), T.gaussian_half_kernel(2.0)
    count, coords, _, dog1 = ops.dog_peaks(dm.float(), w1, w2, 0.1, 3, 512, True)
    link = ops.link_frames(coords, count, 15.0, None)
    ids, lengths, n_tracks = ops.chain_tracks(link, count, None)
    by_hand = dict(zip(("frame", "y", "x", "track_id", "in_long_track"), T._detections_table(coords, count, ids, lengths, 3)))
    by_hand["n_tracks"] = n_tracks
    assert set(table) == set(table0) == set(by_hand)
    for k in by_hand:
        assert torch.equal(table[k], by_hand[k]) and torch.equal(table0[k], by_hand[k]), k
    assert bits_equal(dog.cpu().numpy(), dog1.cpu().numpy()) and bits_equal(dog0.cpu().numpy(), dog1.cpu().numpy())


def test_detector_reaches_estimate_track_diffusion():
    movie, det = _sim()
    dm = movie.cuda()
    torch.manual_seed(0)
    model = M.GeneralTransformer(M.LinearProjectionEmbedding, dict(patch_size=9, embed_dim=64), 64, 4, 128, 1,
                                 partial(M.MLPHead, hidden_dim=128, output_dim=1), F.relu, precision="fp32").cuda()
    loc = {k: det[k] for k in ("gain", "offset", "read_var", "sigma0")}
    kw = dict(patch_size=9, dt=0.03, batch_size=16, min_track_length=5)
    full = T.estimate_track_diffusion(dm, model, 5, localization=loc, detector=det, **kw)
    short = T.estimate_track_diffusion(dm, model, 5, localization=loc, detector={"method": "lrt", "p_fa": 1e-6}, **kw)
    assert len(full["track_id"]) >= 3
    for k in ("track_id", "length", "D_msd"):                              # the camera keys came from localization
        assert torch.equal(full[k], short[k]), k
    with pytest.raises(ValueError, match="keys"):
        T.estimate_track_diffusion(dm, model, 5, detector={"method": "lrt", "fit_sigma": False}, **kw)
