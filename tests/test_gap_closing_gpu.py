"""GPU: the gap-closing kernels (csrc/linking.hip: ops.close_gaps, ops.chain_tracks with gap links) against their numpy
restatement (helpers/tracking.py) -- equality throughout: one algorithm, one order of operations -- and the tracking functions
with max_gap > 0 end to end on a simulated movie with planted dark frames (tests/gap_common.py)."""
import ctypes
import io
from contextlib import redirect_stdout
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gap_common as gc
import linking_common as lc
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import models as M
from moleculardiffusion_mivit_amd.helpers import msd as MSD
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu


def _quiet(fn, *a, **kw):
    with redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.fixture(scope="module")
def joined():
    """The hand case and the drop-out sequence concatenated along F, with movie_start, and the restatement's links."""
    wc, wn = gc.walk_padded()
    cap = wc.shape[1]
    hc = np.zeros((len(gc.HAND_COUNTS), cap, 2), np.int32)
    hc[:, :4] = gc.hand_padded()
    coords, counts = np.concatenate([hc, wc]), np.concatenate([gc.HAND_COUNTS, wn])
    ms = np.zeros(len(counts), np.uint8)
    ms[:7] = gc.HAND_MOVIE_START
    ms[[7, 30, 48]] = 1
    link = T.link_particles_movie(coords, counts, 15, ms)
    return coords, counts, ms, link


def _check_against_restatement(coords, counts, ms, link, max_gap, max_distance=15):
    want_p, want_g = T.close_gaps_movie(coords, counts, link, max_gap, max_distance, ms)
    dc, dn, dl = _dev(coords, counts, link)
    dms = None if ms is None else torch.from_numpy(ms).cuda()
    gp, gf = ops.close_gaps(dc, dn, dl, max_gap, max_distance, dms)
    gp2, gf2 = ops.close_gaps(dc, dn, dl, max_gap, max_distance, dms)
    torch.cuda.synchronize()
    assert gp.dtype == gf.dtype == torch.int32 and gp.shape == gf.shape == link.shape
    assert torch.equal(gp, gp2) and torch.equal(gf, gf2)
    assert np.array_equal(gp.cpu().numpy(), want_p) and np.array_equal(gf.cpu().numpy(), want_g)
    # through the public entry point, and chained
    tp, tg = T.close_gaps_movie(dc, dn, dl, max_gap, max_distance, dms)
    assert torch.equal(tp, gp) and torch.equal(tg, gf)
    ids, lengths, n = ops.chain_tracks(dl, dn, dms, gp, gf)
    wids, wlen, wn = T.chain_tracks(link, counts, ms, want_p, want_g)
    assert np.array_equal(ids.cpu().numpy(), wids) and np.array_equal(lengths.cpu().numpy(), wlen) and int(n) == int(wn[0])
    return want_p, want_g


@pytest.mark.parametrize("max_gap", gc.WALK_MAX_GAPS)
def test_close_gaps_and_chaining_equal_the_restatement(joined, max_gap):
    coords, counts, ms, link = joined
    want_p, want_g = _check_against_restatement(coords, counts, ms, link, max_gap)
    assert (want_g[7:] > 0).sum() > 10
    if max_gap >= gc.HAND_MAX_GAP:                               # (a larger max_gap also closes V's gap of three frames)
        keep = (want_g[:7, :4] > 0) & (want_g[:7, :4] <= gc.HAND_MAX_GAP + 1)
        assert np.array_equal(np.where(keep, want_p[:7, :4], -1), gc.HAND_GAP_PARTNER)
        assert np.array_equal(np.where(keep, want_g[:7, :4], 0), gc.HAND_GAP_FRAMES)
    _check_against_restatement(coords, counts, None, T.link_particles_movie(coords, counts, 15), max_gap)


def test_close_gaps_small_and_empty_shapes(joined):
    coords, counts, ms, link = joined
    for n_frames in (0, 1, 2):
        _check_against_restatement(coords[:n_frames], counts[:n_frames], ms[:n_frames], link[:n_frames], 3)
    # cap = 1: one particle that blinks
    c1 = np.array([[[5, 5]], [[0, 0]], [[6, 7]], [[0, 0]], [[0, 0]], [[8, 8]], [[30, 30]]], np.int32)
    n1 = np.array([1, 0, 1, 0, 0, 1, 1], np.int32)
    l1 = T.link_particles_movie(c1, n1, 15)
    p1, g1 = _check_against_restatement(c1, n1, None, l1, 2)
    assert g1[:, 0].tolist() == [0, 0, 2, 0, 0, 3, 0] and p1[:, 0].tolist() == [-1, -1, 0, -1, -1, 0, -1]
    # empty frames only
    z = np.zeros((5, 3, 2), np.int32)
    _check_against_restatement(z, np.zeros(5, np.int32), None, np.full((5, 3), -1, np.int32), 8)


def test_close_gaps_at_the_capacity_limit_with_few_detections():
    """cap = 1024: the launch asks for the whole LDS plan (63 488 bytes)."""
    cap = ops.LINK_MAX_DETECTIONS
    coords = np.zeros((len(gc.HAND_COUNTS), cap, 2), np.int32)
    coords[:, :4] = gc.hand_padded()
    link = np.full((len(gc.HAND_COUNTS), cap), -1, np.int32)
    link[:, :4] = gc.HAND_LINK
    want_p, want_g = _check_against_restatement(coords, gc.HAND_COUNTS, gc.HAND_MOVIE_START, link, gc.HAND_MAX_GAP)
    assert np.array_equal(want_p[:, :4], gc.HAND_GAP_PARTNER) and np.array_equal(want_g[:, :4], gc.HAND_GAP_FRAMES)
    assert (want_p[:, 4:] == -1).all() and (want_g[:, 4:] == 0).all()


def test_close_gaps_largest_sub_problem_and_chunked_chaining():
    """512 / 0 / 512 detections: pass 2 solves 512 open ends against 512 open starts in one workgroup, and the chain kernel
    walks a frame of more than 256 detections that all carry gap links."""
    a, b = lc.special_cases()["full_512"]
    coords = np.zeros((3, 512, 2), np.int32)
    coords[0], coords[2] = a, b
    counts = np.array([512, 0, 512], np.int32)
    link = T.link_particles_movie(coords, counts, 15)
    assert (link == -1).all()
    want_p, want_g = _check_against_restatement(coords, counts, None, link, 1)
    assert (want_g[2] == 2).sum() > 400 and (want_g[:2] == 0).all()
    ids, _, n = T.chain_tracks(link, counts, None, want_p, want_g)
    assert int(n[0]) == 1024 - int((want_g[2] == 2).sum())
    # with movie_start on the last frame nothing may be closed
    ms = np.array([0, 0, 1], np.uint8)
    blocked_p, blocked_g = _check_against_restatement(coords, counts, ms, link, 1)
    assert (blocked_g == 0).all() and (blocked_p == -1).all()


def test_chain_tracks_ignores_gap_links_that_point_nowhere():
    counts, link, ms = gc.HAND_COUNTS, gc.HAND_LINK, gc.HAND_MOVIE_START
    for p_fill, g_fill in ((3, 2), (0, ops.LINK_MAX_GAP + 2), (-5, 3), (1 << 30, 9), (0, -2), (0, 7)):
        gp, gf = np.full_like(gc.HAND_GAP_PARTNER, p_fill), np.full_like(gc.HAND_GAP_FRAMES, g_fill)
        wids, wlen, wn = T.chain_tracks(link, counts, ms, gp, gf)
        ids, lengths, n = ops.chain_tracks(*_dev(link, counts), torch.from_numpy(ms).cuda(), *_dev(gp, gf))
        assert np.array_equal(ids.cpu().numpy(), wids) and np.array_equal(lengths.cpu().numpy(), wlen) and int(n) == int(wn[0])
    # without gap tensors the old entry runs
    ids, lengths, n = ops.chain_tracks(*_dev(link, counts), torch.from_numpy(ms).cuda())
    wids, wlen, wn = T.chain_tracks(link, counts, ms)
    assert np.array_equal(ids.cpu().numpy(), wids) and np.array_equal(lengths.cpu().numpy(), wlen) and int(n) == int(wn[0])
    e = torch.zeros(0, 4, dtype=torch.int32, device="cuda")
    ids, lengths, n = ops.chain_tracks(e, torch.zeros(0, dtype=torch.int32, device="cuda"), None, e, e)
    assert ids.shape == (0, 4) and lengths.shape == (0,) and int(n) == 0


@pytest.fixture(scope="module")
def sim():
    movie, truth = gc.sim_movie()
    return movie, movie.cuda(), truth


def test_track_particles_tensors_closes_and_fills_the_planted_gaps(sim):
    movie, dm, truth = sim
    table, _ = T.track_particles_tensors(dm, max_gap=2)
    assert set(table) == {"frame", "y", "x", "track_id", "in_long_track", "filled", "n_tracks"}
    assert all(v.is_cuda for v in table.values()) and table["filled"].dtype == torch.bool
    _, det, _ = _quiet(T.track_particles_flat, movie, linking="device", max_gap=2)
    for k in ("frame", "y", "x", "track_id", "filled"):
        assert np.array_equal(table[k].cpu().numpy(), det[k]), k
    tracks, ddet, _ = _quiet(T.track_particles_flat, dm, linking="device", max_gap=2)
    assert all(np.array_equal(ddet[k], det[k]) for k in det)
    assert len(tracks) == gc.SIM_PARTICLES == int(table["n_tracks"])
    fr, y, x, tid, offsets, filled = T.tracks_table_by_track(table)
    assert (offsets[1:] - offsets[:-1]).tolist() == [gc.SIM_FRAMES] * gc.SIM_PARTICLES
    assert torch.equal(fr, torch.arange(gc.SIM_FRAMES, device="cuda").repeat(gc.SIM_PARTICLES))      # gap-free per track
    assert int(filled.sum()) == sum(n for _, _, n in gc.SIM_DARK)
    plain, _ = T.track_particles_tensors(dm, max_gap=0)
    assert "filled" not in plain and int(plain["n_tracks"]) == gc.SIM_PARTICLES + len(gc.SIM_DARK)
    default, _ = T.track_particles_tensors(dm)
    assert all(torch.equal(plain[k], default[k]) for k in default)


def test_estimate_track_diffusion_with_gap_closing(sim):
    movie, dm, truth = sim
    torch.manual_seed(0)
    model = M.GeneralTransformer(M.LinearProjectionEmbedding, dict(patch_size=7, embed_dim=64), 64, 4, 128, 1,
                                 partial(M.MLPHead, hidden_dim=128, output_dim=1), F.relu, precision="fp32").cuda()
    res = T.estimate_track_diffusion(dm, model, seq_len=10, max_gap=2)
    base = T.estimate_track_diffusion(dm, model, seq_len=10, max_gap=0)
    assert "n_filled" not in base and set(res) == set(base) | {"n_filled"}
    assert res["length"].tolist() == [gc.SIM_FRAMES] * gc.SIM_PARTICLES
    # which particle each track follows: the truth position of frame 0
    table, _ = T.track_particles_tensors(dm, max_gap=2, return_dog=False)
    fr, y, x, tid, offsets, filled = T.tracks_table_by_track(table)
    t_y = truth["y"].view(gc.SIM_PARTICLES, gc.SIM_FRAMES)[:, 0]
    t_x = truth["x"].view(gc.SIM_PARTICLES, gc.SIM_FRAMES)[:, 0]
    dark = gc.sim_blink_mask().sum(axis=1)
    want = []
    for k in range(gc.SIM_PARTICLES):
        y0, x0 = float(y[offsets[k]]), float(x[offsets[k]])
        want.append(int(dark[int(torch.argmin((t_y - y0) ** 2 + (t_x - x0) ** 2))]))
    assert res["n_filled"].tolist() == want and sorted(want) == sorted(dark.tolist())
    # D_msd: the host statement on the refined positions the device computed, bitwise
    fit = T.refine_localizations_tensors(T.extract_patches_flat(dm, fr, y, x, 7), y, x)
    pos = torch.stack([fit["y_refined"], fit["x_refined"]], dim=1).cpu().numpy()
    _, want_d, want_w = MSD.track_msd(pos, offsets.cpu().numpy())
    assert np.array_equal(res["D_msd"].cpu().numpy().view(np.int64), want_d.view(np.int64))
    assert np.array_equal(res["D_msd_weighted"].cpu().numpy().view(np.int64), want_w.view(np.int64))
    # a filled row on a dark frame has nothing to fit: the interpolated position stands where the fit fails
    failed = fit["status"] != 0
    assert torch.equal(fit["y_refined"][failed], y[failed].double())
    assert int(res["n_sequences"].sum()) == gc.SIM_PARTICLES * (gc.SIM_FRAMES // 10) > int(base["n_sequences"].sum())
    assert bool(torch.isfinite(res["D_model"]).all())


def test_entry_point_errors():
    coords, counts, link = _dev(gc.hand_padded(), gc.HAND_COUNTS, gc.HAND_LINK)
    gp, gf = _dev(gc.HAND_GAP_PARTNER, gc.HAND_GAP_FRAMES)
    with pytest.raises(ValueError, match="int32 GPU tensor"):
        ops.close_gaps(coords.long(), counts, link, 2)
    with pytest.raises(ValueError, match="int32 GPU tensor"):
        ops.close_gaps(coords.cpu(), counts, link, 2)
    with pytest.raises(ValueError, match="link must be"):
        ops.close_gaps(coords, counts, link.long(), 2)
    with pytest.raises(ValueError, match="link must be"):
        ops.close_gaps(coords, counts, link.cpu(), 2)
    with pytest.raises(ValueError, match="link must be"):
        ops.close_gaps(coords, counts, link[:, :3], 2)
    with pytest.raises(ValueError, match="count must be"):
        ops.close_gaps(coords, counts[:3], link, 2)
    with pytest.raises(ValueError, match="movie_start"):
        ops.close_gaps(coords, counts, link, 2, movie_start=[1, 0])
    for bad in (0, -1, ops.LINK_MAX_GAP + 1, 1.5, None):
        with pytest.raises(ValueError, match="LINK_MAX_GAP"):
            ops.close_gaps(coords, counts, link, bad)
    with pytest.raises(ValueError, match="NaN"):
        ops.close_gaps(coords, counts, link, 2, float("nan"))
    with pytest.raises(ValueError, match="both"):
        ops.chain_tracks(link, counts, None, gp)
    with pytest.raises(ValueError, match="gap_frames must be"):
        ops.chain_tracks(link, counts, None, gp, gf.long())
    with pytest.raises(ValueError, match="gap_partner must be"):
        ops.chain_tracks(link, counts, None, gp[:3], gf)
    with pytest.raises(ValueError, match="gap_partner must be"):
        ops.chain_tracks(link, counts, None, gp.cpu(), gf)
    with pytest.raises(ValueError, match="CUDA movie"):
        T.track_particles_tensors(torch.zeros(4, 32, 32), max_gap=1)
    with pytest.raises(ValueError, match="max_gap"):
        T.track_particles_tensors(torch.zeros(4, 32, 32, device="cuda"), max_gap=ops.LINK_MAX_GAP + 1)
    # the C entries validate before any launch
    from moleculardiffusion_mivit_amd import _native as N
    big = ops.LINK_MAX_DETECTIONS + 1
    vp = ctypes.c_void_p
    fake = vp(0x1000)                               # never dereferenced: validation comes first
    rc = N.lib.mivit_close_gaps(fake, fake, fake, None, 2, big, 2, 15.0, fake, fake, fake, 2 * big, None)
    assert rc != 0 and "capacity" in N.last_error()
    rc = N.lib.mivit_close_gaps(fake, fake, fake, None, 2, 4, 9, 15.0, fake, fake, fake, 8, None)
    assert rc != 0 and "max_gap" in N.last_error()
    rc = N.lib.mivit_close_gaps(fake, fake, fake, None, 2, 4, 2, 15.0, fake, fake, fake, 7, None)
    assert rc != 0 and "workspace" in N.last_error()
    rc = N.lib.mivit_chain_tracks_gaps(fake, fake, fake, fake, None, 2, big, 2, fake, fake, fake, None)
    assert rc != 0 and "capacity" in N.last_error()
    rc = N.lib.mivit_chain_tracks_gaps(fake, fake, fake, fake, None, 2, 4, 0, fake, fake, fake, None)
    assert rc != 0 and "max_gap" in N.last_error()
