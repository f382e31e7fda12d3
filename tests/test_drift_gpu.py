"""GPU: the kernels of csrc/drift.hip (ops.drift_frames in both modes, ops.drift_integrate) against the numpy restatements of
helpers/msd.py, BIT FOR BIT -- no transcendental function is involved -- on the common set of tests/drift_common.py, which
tests/test_drift.py holds against an independent oracle; and the paths that reach them: helpers/msd.estimate_drift on CUDA
tensors and tracking.estimate_track_diffusion(drift=...)."""
import numpy as np
import pytest
import torch

import drift_common as dc
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as msd_mod
from moleculardiffusion_mivit_amd.helpers import tracking as trk

pytestmark = pytest.mark.gpu

H = dc.HALF_WINDOW
MODES = ("mean", "median")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                 # a copy: the common inputs are read-only


def _pairs(min_pairs=1):
    """The pair list of the common table, built on the device -> (pos, pair_row int32, frame_offsets int32, n_pairs int32)."""
    pos, frames, offsets, use = (_dev(a) for a in dc.common_table())
    rows, counts, fo, rejected = msd_mod._drift_pairs(pos, frames, offsets, use, dc.N_FRAMES, min_pairs)
    assert rejected == dc.N_REJECTED
    return pos, rows.int(), fo.int(), counts.int()


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(dc.bits(got), dc.bits(want)), (what, np.argwhere(dc.bits(got) != dc.bits(want))[:5])


@pytest.mark.parametrize("min_pairs", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_drift_frames_is_bitwise_the_restatement(mode, min_pairs):
    pos, rows, fo, counts = _pairs(min_pairs)
    assert counts.cpu().tolist() == [0 if c < min_pairs else c for c in (dc.FRAME_PAIRS.get(f, 0) for f in range(dc.N_FRAMES))]
    want = msd_mod._drift_frames_numpy(pos.cpu().numpy(), rows.cpu().numpy(), fo.cpu().numpy(), ops.DRIFT_MODES[mode])
    got = ops.drift_frames(pos, rows, fo, mode)
    _same(got, want, mode)
    _same(ops.drift_frames(pos, rows, fo, ops.DRIFT_MODES[mode]), want, "the mode as a number")
    _same(ops.drift_frames(pos, rows, fo, mode), want, "a second call gives the same bits")


@pytest.mark.parametrize("mode", MODES)
def test_a_frame_alone_gives_the_bits_it_has_in_the_batch(mode):
    pos, rows, fo, _ = _pairs()
    full = ops.drift_frames(pos, rows, fo, mode).cpu().numpy()
    fo_h = fo.cpu().numpy()
    for f in range(dc.N_FRAMES):
        a, b = int(fo_h[f]), int(fo_h[f + 1])
        alone = ops.drift_frames(pos, rows[a:b].contiguous(), _dev(np.array([0, b - a], np.int32)), mode)
        _same(alone, full[f:f + 1], (mode, f))
    # the frames in reverse order: the same rows of stat, reversed
    order = list(range(dc.N_FRAMES))[::-1]
    r2 = torch.cat([rows[int(fo_h[f]):int(fo_h[f + 1])] for f in order]).contiguous()
    fo2 = _dev(np.concatenate([[0], np.cumsum([fo_h[f + 1] - fo_h[f] for f in order])]).astype(np.int32))
    _same(ops.drift_frames(pos, r2, fo2, mode), full[::-1].copy(), (mode, "reversed"))


@pytest.mark.parametrize("F,h", [(F, h) for F in dc.INTEGRATE_F for h in (0, 1, H)] + [(2 * H + 1, 50), (257, 300)])
def test_drift_integrate_is_bitwise_the_restatement(F, h):
    stat, n = dc.integrate_case(F)
    wv, wd = msd_mod._drift_integrate_numpy(stat, n, h)
    vel, drift = ops.drift_integrate(_dev(stat), _dev(n), h)
    _same(vel, wv, ("velocity", F, h))
    _same(drift, wd, ("drift", F, h))
    again = ops.drift_integrate(_dev(stat), _dev(n), h)
    _same(again[0], wv, "repeat")
    _same(again[1], wd, "repeat")
    if h == 0 and F > 1:
        _same(vel[1:], stat[1:], "h = 0: stat itself")


def test_integrate_on_the_common_tables_statistics():
    pos, rows, fo, counts = _pairs()
    for mode in MODES:
        stat = ops.drift_frames(pos, rows, fo, mode)
        for h in (0, H):
            wv, wd = msd_mod._drift_integrate_numpy(stat.cpu().numpy(), counts.cpu().numpy(), h)
            vel, drift = ops.drift_integrate(stat, counts, h)
            _same(vel, wv, (mode, h))
            _same(drift, wd, (mode, h))


def test_wrappers_reject_before_any_launch():
    pos, rows, fo, counts = _pairs()
    # one pair more than the median sorts: a ValueError of the wrapper; the mean takes the same frame
    n = ops.DRIFT_MAX_PAIRS + 1
    big_pos = torch.arange(2 * (n + 1), dtype=torch.float64, device="cuda").view(n + 1, 2) * 0.5
    big_rows = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    big_fo = _dev(np.array([0, n], np.int32))
    with pytest.raises(ValueError, match="DRIFT_MAX_PAIRS"):
        ops.drift_frames(big_pos, big_rows, big_fo, "median")
    _same(ops.drift_frames(big_pos, big_rows, big_fo, "mean"), np.array([[1.0, 1.0]]), "the mean has no limit")
    at_limit = ops.drift_frames(big_pos, big_rows[:-1].contiguous(), _dev(np.array([0, n - 1], np.int32)), "median")
    _same(at_limit, np.array([[1.0, 1.0]]), "DRIFT_MAX_PAIRS pairs are sorted")
    # the C entry rejects it as well, before any HIP call
    assert N.lib.mivit_drift_frames(None, n + 1, None, n, None, 1, 1, n, None, None) != 0
    assert N.lib.mivit_drift_frames(None, 0, None, 0, None, 0, 0, 0, None, None) == 0     # no frames: a no-op
    assert N.lib.mivit_drift_frames(None, 4, None, 0, None, 1, 2, 0, None, None) != 0     # no such mode
    assert N.lib.mivit_drift_integrate(None, None, 0, 0, None, None, None) == 0
    assert N.lib.mivit_drift_integrate(None, None, 4, -1, None, None, None) != 0
    bad = [
        (lambda: ops.drift_frames(pos.float(), rows, fo), "pos"), (lambda: ops.drift_frames(pos.cpu(), rows, fo), "pos"),
        (lambda: ops.drift_frames(pos, rows.long(), fo), "pair_row"), (lambda: ops.drift_frames(pos, rows, fo.long()), "frame_offsets"),
        (lambda: ops.drift_frames(pos, rows, fo[:-2].contiguous()), "rise from 0"),    # the last frame is empty: cut one more
        (lambda: ops.drift_frames(pos, rows, fo, "mode"), "mode"), (lambda: ops.drift_frames(pos, rows, fo, 2), "mode"),
        (lambda: ops.drift_frames(pos, torch.zeros_like(rows), fo), r"pair_row must lie in"),
        (lambda: ops.drift_frames(pos, rows + pos.shape[0], fo), r"pair_row must lie in"),
        (lambda: ops.drift_frames(pos[:, :1].contiguous(), rows, fo), r"\[N, 2\]"),
        (lambda: ops.drift_integrate(torch.zeros(4, 2, device="cuda"), counts[:4].contiguous()), "stat"),
        (lambda: ops.drift_integrate(torch.zeros(4, 2, dtype=torch.float64, device="cuda"), counts[:5].contiguous()), "n_pairs"),
        (lambda: ops.drift_integrate(torch.zeros(4, 2, dtype=torch.float64, device="cuda"), counts[:4].contiguous(), -1), "half_window"),
        (lambda: ops.drift_integrate(torch.zeros(4, 2, dtype=torch.float64, device="cuda"), counts[:4].contiguous(), 1.5), "half_window"),
    ]
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
    empty = ops.drift_frames(pos, rows[:0].contiguous(), _dev(np.zeros(4, np.int32)))
    _same(empty, np.zeros((3, 2)), "frames without pairs")


@pytest.mark.parametrize("estimator", MODES)
def test_estimate_drift_on_cuda_tensors_equals_the_cpu_call(estimator):
    pos, frames, offsets, use = dc.common_table()
    for kw in (dict(), dict(smoothing=H, min_pairs=2), dict(smoothing=1, n_frames=dc.N_FRAMES + 3)):
        want = msd_mod.estimate_drift(pos, frames, offsets, estimator=estimator, use=use, **kw)
        got = msd_mod.estimate_drift(_dev(pos), _dev(frames), _dev(offsets), estimator=estimator, use=_dev(use), **kw)
        assert got["n_rejected"] == want["n_rejected"] == dc.N_REJECTED
        for k in ("drift", "velocity", "n_pairs"):
            assert got[k].is_cuda
            _same(got[k], want[k], (estimator, k, kw))
    with pytest.raises(ValueError, match="DRIFT_MAX_PAIRS"):               # CUDA only: the restatement has no limit
        n = ops.DRIFT_MAX_PAIRS + 1
        p = torch.zeros(2 * n, 2, dtype=torch.float64, device="cuda")
        msd_mod.estimate_drift(p, torch.arange(2, device="cuda").repeat(n), torch.arange(0, 2 * n + 1, 2, device="cuda"),
                               estimator="median")


class MeanPixel(torch.nn.Module):
    def forward(self, seq):
        return seq.mean(dim=(1, 2, 3)).unsqueeze(1)


def _same_t(a, b):
    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


def test_end_to_end_on_a_drifting_movie():
    """64 x 64, 40 frames, 12 particles that live through the movie, D = 0.05, noise-free, on a stage that moves 0.5 pixels a
    frame in x.  Uncorrected, the lag-1 MSD carries v^2 = 0.25 on top of 4 D = 0.2 and the later lags v^2 k^2: D_msd is off by
    far more than a factor two, and the correction must bring the median error over the tracks below the uncorrected one."""
    Np, F_, D, v = 12, 40, 0.05, (0.0, 0.5)
    props = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
    g = torch.Generator(device="cuda").manual_seed(7)
    # the stage moves 19.5 pixels in x: a particle that starts in the right third leaves the field and its track ends early
    movie, truth = gen.simulate_movie(Np, F_, 64, 64, (D, 0.0), 2, image_props=props, generator=g, device="cuda", drift=v)
    model = MeanPixel().cuda()
    base = trk.estimate_track_diffusion(movie, model, 10)
    res = trk.estimate_track_diffusion(movie, model, 10, drift={})
    assert set(res) == set(base) | {"drift"}
    for k in ("track_id", "length", "n_sequences", "D_model"):             # the tracks and the model's numbers do not change
        assert _same_t(base[k], res[k]), k
    # the stages, rebuilt: the drift is estimate_drift on the refined positions, and the MSD that of the corrected ones
    table, _ = trk.track_particles_tensors(movie, return_dog=False)
    fr, y, x, tid, offsets = trk.tracks_table_by_track(table)[:5]
    fit = trk.refine_localizations_tensors(trk.extract_patches_flat(movie.float(), fr, y, x, 7), y, x)
    pos = torch.stack([fit["y_refined"], fit["x_refined"]], dim=1)
    by_hand = msd_mod.estimate_drift(pos, fr, offsets, n_frames=F_)
    dr = res["drift"]
    assert set(dr) == set(by_hand) | {"positions"} and dr["n_rejected"] == by_hand["n_rejected"] == 0
    for k in ("drift", "velocity", "n_pairs"):
        assert _same_t(dr[k], by_hand[k]), k
    corrected = msd_mod.subtract_drift(pos, fr, by_hand["drift"])
    assert _same_t(dr["positions"], corrected)
    msd, d_lstsq, d_weighted = ops.track_msd(corrected, offsets.int(), 1.0, 0)
    assert _same_t(res["msd"], msd) and _same_t(res["D_msd"], d_lstsq) and _same_t(res["D_msd_weighted"], d_weighted)
    # a call without drift is what it was: the MSD of the uncorrected positions
    msd0, d0, w0 = ops.track_msd(pos, offsets.int(), 1.0, 0)
    assert _same_t(base["msd"], msd0) and _same_t(base["D_msd"], d0) and _same_t(base["D_msd_weighted"], w0)
    n_tracks = len(res["track_id"])
    assert n_tracks >= 8, f"tracking recovered {n_tracks} tracks of {Np} particles"
    assert not bool(torch.isnan(base["D_msd"]).any() | torch.isnan(res["D_msd"]).any())
    err0 = float((base["D_msd"] - D).abs().median())
    err1 = float((res["D_msd"] - D).abs().median())
    vel = dr["velocity"][1:].mean(dim=0)
    print(f"{n_tracks} tracks; median |D_msd - D|: {err0:.4f} uncorrected, {err1:.4f} corrected; mean velocity {vel.tolist()}")
    assert err1 < err0
    # with the other options: segment and states run on the corrected positions
    both = trk.estimate_track_diffusion(movie, model, 10, drift={"estimator": "median", "smoothing": 2}, segment={})
    seg = msd_mod.segment_tracks(both["drift"]["positions"], offsets, dt=1.0)
    assert all(_same_t(seg[k], both["segments"][k]) for k in seg)


def test_filled_rows_of_gap_closed_tracks_stay_out_of_the_estimate():
    """A blinking movie with gap closing: the rows fill_gaps adds carry interpolated positions, and the drift is estimated
    without them (use = ~filled), on the refined positions, exactly as estimate_drift gives it by hand."""
    Np, F_ = 10, 40
    props = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
    g = torch.Generator(device="cuda").manual_seed(3)
    movie, _ = gen.simulate_movie(Np, F_, 64, 64, (0.05, 0.0), 2, image_props=props, generator=g, device="cuda", blink=0.15,
                                  drift=(0.1, -0.2))
    res = trk.estimate_track_diffusion(movie, MeanPixel().cuda(), 10, max_gap=2, drift={"estimator": "median"})
    table, _ = trk.track_particles_tensors(movie, return_dog=False, max_gap=2)
    fr, y, x, tid, offsets, filled = trk.tracks_table_by_track(table)
    assert int(filled.sum()) > 0 and int(res["n_filled"].sum()) == int(filled.sum())
    fit = trk.refine_localizations_tensors(trk.extract_patches_flat(movie.float(), fr, y, x, 7), y, x)
    pos = torch.stack([fit["y_refined"], fit["x_refined"]], dim=1)
    by_hand = msd_mod.estimate_drift(pos, fr, offsets, n_frames=F_, estimator="median", use=~filled)
    unmasked = msd_mod.estimate_drift(pos, fr, offsets, n_frames=F_, estimator="median")
    for k in ("drift", "velocity", "n_pairs"):
        assert _same_t(res["drift"][k], by_hand[k]), k
    assert int(by_hand["n_pairs"].sum()) < int(unmasked["n_pairs"].sum())
    assert _same_t(res["drift"]["positions"], msd_mod.subtract_drift(pos, fr, by_hand["drift"]))
