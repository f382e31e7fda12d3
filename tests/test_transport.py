"""CPU: the numpy restatements of csrc/segment.hip (helpers/msd._transport_numpy, _transport_stats_numpy) against the oracle
and the formulas of tests/transport_common.py, the statistics of the segmenter on planted run-and-pause tracks and on free
walks, the front end helpers/msd.segment_transport, and the simulator's per-state velocities (generation.multi_state,
simulate_movie(states={..., "velocity": ...})).  No kernel is launched here; tests/test_transport_gpu.py holds the kernels
against these restatements.

tracking.estimate_track_diffusion refuses a movie that is not on the GPU, so what transport= adds to its result is checked in
tests/test_transport_gpu.py; here its argument check (which precedes that refusal) and transport_per_track are."""
import math

import numpy as np
import pytest
import torch

import transport_common as tc
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as msd_mod
from moleculardiffusion_mivit_amd.helpers import tracking as trk


def _restated(mode, margin=False):
    pos, offsets, _ = tc.common_tracks()
    return msd_mod._transport_numpy(pos, offsets, tc.MIN_LEN, tc.PENALTY, tc.VELOCITY_PENALTY, tc.MIN_VAR, mode, return_margin=margin)


@pytest.mark.parametrize("mode", sorted(tc.MODES))
def test_restatement_equals_the_oracle_on_every_track(mode):
    pos, offsets, plant = tc.common_tracks()
    m = tc.MODES[mode]
    seg_start, seg_class, cost = _restated(m)
    want_cuts, want_classes, want_cost = tc.oracle_common(m)
    assert len(offsets) - 1 == tc.N_TRACKS
    got_cuts, got_classes = tc.partition_of(seg_start, seg_class, offsets)
    for k in range(tc.N_TRACKS):
        assert got_cuts[k] == want_cuts[k] and got_classes[k] == want_classes[k], (k, got_cuts[k], want_cuts[k], got_classes[k], want_classes[k])
    assert np.array_equal(np.isnan(cost), np.isnan(want_cost))
    ok = ~np.isnan(cost)
    assert list(np.nonzero(~ok)[0]) == [0, 5]                              # the one-row track and the empty one
    err = np.abs(cost[ok] - want_cost[ok]) / (1 + np.abs(want_cost[ok]))
    print(f"{mode}: worst |cost - oracle| / (1 + |cost|) = {err.max():.3g}")
    assert err.max() <= tc.COST_RTOL
    for k in np.nonzero(ok)[0]:                                            # the restatement's partition, scored by the oracle
        rescored = tc.score_partition(pos[offsets[k]:offsets[k + 1]], got_cuts[k], got_classes[k], m)
        assert abs(rescored - want_cost[k]) <= tc.COST_RTOL * (1 + abs(want_cost[k])), k
    if mode == "both":                                                     # what was planted at 3 step sd per frame is found
        found = 0
        for k, (cuts, classes) in plant.items():
            if k < tc.N_TRACKS - 6:
                assert got_classes[k] == classes and len(got_cuts[k]) == len(cuts), k
                assert all(abs(a - b) <= 5 for a, b in zip(got_cuts[k], cuts)), (k, got_cuts[k], cuts)
                found += 1
        assert found == 6


def test_every_common_track_has_a_margin():
    """What lets tests/test_transport_gpu.py compare partitions and classes EXACTLY."""
    for mode, m in tc.MODES.items():
        margin = _restated(m, margin=True)[3]
        print(f"{mode}: smallest margin {margin.min():.3g}")
        assert (margin >= tc.MIN_MARGIN).all(), (mode, np.nonzero(margin < tc.MIN_MARGIN)[0], margin.min())
    never_moves = tc.N_TRACKS - 13
    seg_start, seg_class, cost = _restated(0)
    pos, offsets, _ = tc.common_tracks()
    a, b = offsets[never_moves], offsets[never_moves + 1]
    assert seg_start[a:b].sum() == 1 and seg_class[a:b].sum() == 0         # both costs at the floor: the tie is diffusive
    assert abs(cost[never_moves] - 2 * 19 * math.log(tc.MIN_VAR)) < 1e-9


def test_diffusive_mode_is_segment_tracks_bit_for_bit():
    pos, offsets, _ = tc.common_tracks()
    seg_start, seg_class, cost = _restated(2)
    want_start, want_cost = msd_mod._segment_numpy(pos, offsets, tc.MIN_LEN, tc.PENALTY, tc.MIN_VAR)
    assert np.array_equal(seg_start, want_start) and not seg_class.any()
    assert np.array_equal(cost.view(np.int64), want_cost.view(np.int64))


def test_directed_mode_is_galilean_invariant():
    """A velocity of 10 step standard deviations per frame added to the planted tracks leaves every partition as it is: the
    sums are not centred, so SS - S^2 / n cancels, but harmlessly.  Bound of the cost's change: the residual of a stretch of n
    increments is about 2 n sd^2 and SS about n (v^2 + 2 sd^2) = 51 times that; cs2[j] carries a rounding of at most j ulp of
    itself, j <= 240, and cs2[j] <= 240 * 102 sd^2, against a residual of at least min_len * 2 sd^2 / a few: a relative error of
    the residual of 240 * (240 * 102 / 8) * 1.1e-16 * a few = 1e-10 at the very worst, which log turns into an absolute error
    that 2 n multiplies: 5e-8 on costs of magnitude 100 .. 1000.  1e-9 * (1 + |cost|) is that bound; measured: see the print
    (DESIGN 4v records it)."""
    pos, offsets, plant = tc.common_tracks()
    v = 10.0 * tc.STEP_SD * np.array([math.sin(0.6), math.cos(0.6)])
    worst = 0.0
    for k in plant:
        p = pos[offsets[k]:offsets[k + 1]]
        off = np.array([0, len(p)], np.int64)
        moved = p + np.arange(len(p))[:, None] * v[None, :]
        a = msd_mod._transport_numpy(p, off, tc.MIN_LEN, tc.PENALTY, tc.VELOCITY_PENALTY, tc.MIN_VAR, 1)
        b = msd_mod._transport_numpy(moved, off, tc.MIN_LEN, tc.PENALTY, tc.VELOCITY_PENALTY, tc.MIN_VAR, 1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and b[1].all(), k
        worst = max(worst, abs(a[2][0] - b[2][0]) / (1 + abs(a[2][0])))
    print(f"directed mode, + 10 sd per frame on {len(plant)} planted tracks: partitions equal, worst relative cost change {worst:.3g}")
    assert worst <= 1e-9


def test_statistics_on_planted_runs_and_on_free_walks():
    """The defaults (penalty = velocity_penalty = 3, min_len = 4) at fixed seeds.  Planted: 60 tracks of three stretches of 40
    increments that alternate pause and run, D = 0.05, run speed 2 sqrt(2 D) per frame in a random direction; at least 48 of
    60 must have exactly two cuts, each within 5 of its planted place, and all three classes right.  Null: 100 free walks of
    100 increments; at most 5 may get a directed stretch.  Measured: see the prints (DESIGN 4v records them)."""
    rng = np.random.default_rng(7)
    right = 0
    for t in range(60):
        p, cuts, classes, _ = tc.run_and_pause(rng, 2, 2.0, 40, start_run=t % 2 == 1, D=0.05)
        out = msd_mod.segment_transport(p, np.array([0, len(p)]))
        got = out["seg_offsets"][1:-1].tolist()
        right += len(got) == 2 and all(abs(a - b) <= 5 for a, b in zip(got, cuts)) and out["seg_class"].tolist() == classes
    print(f"planted: {right} of 60 tracks have their two cuts within 5 increments and their three classes right")
    assert right >= 48
    rng = np.random.default_rng(8)
    directed = cut = 0
    for t in range(100):
        p = tc.brownian(rng, 101, 0.05)
        out = msd_mod.segment_transport(p, np.array([0, len(p)]))
        directed += bool(out["seg_class"].any())
        cut += len(out["seg_track"]) > 1
    print(f"null: {directed} of 100 free walks get a directed stretch, {cut} get a cut")
    assert directed <= 5


def test_stats_restatement_against_the_formulas():
    pos, offsets, _ = tc.common_tracks()
    seg_start = _restated(0)[0]
    first = np.nonzero(seg_start)[0]
    seg_offsets = np.concatenate([first, [len(pos)]]).astype(np.int64)
    seg_track = np.searchsorted(offsets, first, side="right") - 1
    track_end = offsets[seg_track + 1]
    for dt, R in ((1.0, 0.0), (0.05, 1.0 / 6.0)):
        vel, d_res, d_cve, sigma2, n_inc = msd_mod._transport_stats_numpy(pos, seg_offsets, track_end, dt, R)
        for s in range(len(first)):
            hi = min(seg_offsets[s + 1], track_end[s] - 1)
            want = tc.direct_stats(pos[seg_offsets[s]:hi + 1], dt, R)
            assert n_inc[s] == max(hi - seg_offsets[s], 0)
            got = (vel[s, 0], vel[s, 1], d_res[s], d_cve[s], sigma2[s])
            flat = (want[0][0], want[0][1]) + want[1:]
            for g, w in zip(got, flat):
                assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-11 * (abs(w) + 1e-3), (s, got, flat)
    # by hand: 0, 1 and 2 increments, and a stretch that ends its track
    seg_offsets = np.array([0, 1, 2, 4, 9, 9, 40], np.int64)
    track_end = np.array([9, 9, 9, 9, 40, 40], np.int64)
    vel, d_res, d_cve, sigma2, n_inc = msd_mod._transport_stats_numpy(pos[:40], seg_offsets, track_end, 0.5, 0.1)
    assert n_inc.tolist() == [1, 1, 2, 4, 0, 30]
    assert np.isnan(d_cve[:2]).all() and (d_res[:2] == 0).all() and not np.isnan(vel[:2]).any()      # one increment is its own mean
    assert np.isnan(vel[4]).all() and np.isnan(d_res[4]) and not np.isnan(d_cve[[2, 3, 5]]).any()
    # a constant velocity is removed: the estimates of a walk do not see it
    rng = np.random.default_rng(5)
    p = tc.brownian(rng, 200, 0.2)
    moved = p + np.arange(200)[:, None] * np.array([0.7, -1.3])[None, :]
    off, end = np.array([0, 200], np.int64), np.array([200], np.int64)
    a, b = msd_mod._transport_stats_numpy(p, off, end, 1.0, 0.0), msd_mod._transport_stats_numpy(moved, off, end, 1.0, 0.0)
    assert np.allclose(b[0] - a[0], [[0.7, -1.3]], rtol=0, atol=1e-12)
    for x, y in zip(a[1:4], b[1:4]):
        assert np.allclose(x, y, rtol=1e-10, atol=0)


def test_front_end_on_arrays_and_cpu_tensors():
    pos, offsets, _ = tc.common_tracks()
    out = msd_mod.segment_transport(pos, offsets, dt=0.5, blur=0.1)
    n_seg = len(out["seg_track"])
    assert set(out) == {"seg_offsets", "seg_track", "seg_class", "velocity", "speed", "D_res", "D_cve", "sigma2", "n_increments", "cost"}
    assert out["seg_offsets"].shape == (n_seg + 1,) and out["velocity"].shape == (n_seg, 2) and out["cost"].shape == (tc.N_TRACKS,)
    for k in ("seg_class", "speed", "D_res", "D_cve", "sigma2", "n_increments"):
        assert out[k].shape == (n_seg,), k
    assert np.array_equal(out["speed"], np.sqrt(out["velocity"][:, 0] ** 2 + out["velocity"][:, 1] ** 2), equal_nan=True)
    assert np.isnan(out["speed"]).sum() == 1                               # the one-row track: a stretch without an increment
    seg_start, seg_class, cost = _restated(0)
    assert np.array_equal(out["seg_offsets"][:-1], np.nonzero(seg_start)[0]) and np.array_equal(out["seg_class"], seg_class[seg_start == 1])
    as_t = msd_mod.segment_transport(torch.from_numpy(pos.copy()), torch.from_numpy(offsets.copy()), dt=0.5, blur=0.1)
    for k, v in out.items():
        assert torch.is_tensor(as_t[k]) and np.array_equal(as_t[k].numpy(), v, equal_nan=True), k
    for kw in ({"min_len": 1}, {"penalty": -1.0}, {"velocity_penalty": -1.0}, {"velocity_penalty": float("nan")}, {"min_var": 0.0},
               {"classes": "runs"}, {"classes": 1}, {"dt": 0.0}, {"blur": 0.3}):
        with pytest.raises(ValueError):
            msd_mod.segment_transport(pos, offsets, **kw)
    with pytest.raises(ValueError):
        msd_mod.segment_transport(pos, torch.from_numpy(offsets.copy()))
    with pytest.raises(ValueError):
        msd_mod.segment_transport(pos[:, :1], offsets)


def _same(a, b):
    if torch.is_tensor(a):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                         b.view(torch.int32) if b.dtype == torch.float32 else b)
    return a == b


def test_simulator_state_velocities():
    Np, F_, npos = 5, 24, 3
    path = torch.from_numpy(tc.planted_path(Np, F_, 10))
    props = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
    base_states = {"Ds": (0.05, 0.05), "M": np.eye(2), "path": path}

    def movie(states, **kw):
        return gen.simulate_movie(Np, F_, 48, 48, None, npos, image_props=props, generator=torch.Generator().manual_seed(3),
                                  states=states, **kw)

    vid0, truth0 = movie(base_states)
    vidz, truthz = movie(dict(base_states, velocity=np.zeros((2, 2))))
    assert torch.equal(vid0, vidz) and set(truthz) == set(truth0) | {"velocity_row"}
    for k in truth0:                                                       # all zeros: the movie and the truth of no key
        assert _same(truth0[k], truthz[k]), k
    assert not truthz["velocity_row"].any() and truthz["velocity_row"].shape == (Np * F_, 2)
    V = torch.tensor([[0.0, 0.0], [0.3, -0.6]], dtype=torch.float64)
    vid, truth = movie(dict(base_states, velocity=V))
    assert torch.equal(truth["velocity_row"], V[truth["state"]]) and truth["velocity_row"].dtype == torch.float64
    for k in ("state", "D_row", "D", "amp", "frame", "particle_id"):
        assert _same(truth0[k], truth[k]), k
    # the displacement: V[state] / npos per sub-step from sub-step 1 on, accumulated along the path
    inc = (V[path] / npos).repeat_interleave(npos, dim=1)
    inc[:, 0] = 0.0
    want = torch.cumsum(inc, dim=1)
    moved = truth["pos"].double() - truth0["pos"].double()
    assert float((moved - want).abs().max()) <= 2 * 48 * 2.0 ** -24        # both float32 positions round once, below 48 pixels
    frames_in_state = torch.stack([(path == k).sum(dim=1) for k in range(2)], dim=1).double()           # [Np, 2]
    total = frames_in_state @ V - V[path[:, 0]] / npos                     # sub-step 0 stays at the start
    assert float((moved[:, -1] - total).abs().max()) <= 2 * 48 * 2.0 ** -24
    assert float((moved[1, -1] - V[1] * 10 + V[1] / npos).abs().max()) <= 1e-5      # an odd particle runs for 10 frames
    assert not torch.equal(vid, vid0)
    from moleculardiffusion_mivit_amd.helpers import geometry
    filament = geometry.Geometry([geometry.Edge((12.0, 12.0), (30.0, 30.0))])
    movie(base_states, geometry=filament)                                  # fine without the key
    for kw in ({"velocity": (0.1, 0.0)}, {"confinement": {"radius": 2.0}}, {"geometry": filament}):
        with pytest.raises(ValueError, match="velocity"):
            movie(dict(base_states, velocity=V), **kw)
    for bad in (np.zeros((3, 2)), np.zeros(2), [[0.0, float("nan")], [0.0, 0.0]], "fast"):
        with pytest.raises(ValueError):
            movie(dict(base_states, velocity=bad))
    # multi_state: None and zeros are today's trajectories; a velocity displaces by V dt per step in the state
    M = [[0.9, 0.1], [0.2, 0.8]]
    t0, s0 = gen.multi_state(7, 50, (0.05, 0.05), M, dt=0.5, generator=torch.Generator().manual_seed(4))
    tz, sz = gen.multi_state(7, 50, (0.05, 0.05), M, dt=0.5, generator=torch.Generator().manual_seed(4), velocities=np.zeros((2, 2)))
    tv, sv = gen.multi_state(7, 50, (0.05, 0.05), M, dt=0.5, generator=torch.Generator().manual_seed(4), velocities=V)
    assert _same(t0, tz) and torch.equal(s0, sz) and torch.equal(s0, sv) and tv.dtype == t0.dtype and tv.shape == t0.shape
    inc = V[s0] * 0.5
    inc[:, 0] = 0.0
    assert float((tv.double() - t0.double() - torch.cumsum(inc, dim=1).transpose(0, 1)).abs().max()) <= 1e-5
    with pytest.raises(ValueError):
        gen.multi_state(7, 50, (0.05, 0.05), M, velocities=np.zeros((3, 2)))


def test_track_level_summary_and_the_transport_argument():
    seg_offsets = torch.tensor([0, 10, 25, 40, 40 + 7, 60])
    seg_track = torch.tensor([0, 0, 0, 2, 2])
    seg_class = torch.tensor([0, 1, 0, 1, 1])
    lengths = torch.tensor([40, 0, 20])
    frac, runs = trk.transport_per_track(seg_offsets, seg_track, seg_class, lengths)
    assert frac.dtype == torch.float64 and runs.dtype == torch.int64
    assert frac[0] == 15 / 40 and math.isnan(float(frac[1])) and frac[2] == 1.0 and runs.tolist() == [1, 0, 2]
    movie = torch.zeros(4, 16, 16)
    for bad in ({"speed": 1.0}, [], "both"):                               # refused before anything else is looked at
        with pytest.raises(ValueError, match="transport"):
            trk.estimate_track_diffusion(movie, torch.nn.Identity(), 4, transport=bad)
