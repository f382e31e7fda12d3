"""CPU: gap closing (helpers/tracking.py: close_gaps_movie, chain_tracks with gap links, fill_gaps, the max_gap argument of
the tracking functions) and blinking in the simulator (helpers/generation.simulate_movie).  The restatement is held against
the hand-written case and the planted scenes of tests/gap_common.py, and against the structure the definition implies; the
kernels are held against the restatement in tests/test_gap_closing_gpu.py."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import gap_common as gc
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as MSD
from moleculardiffusion_mivit_amd.helpers import tracking as T


def _quiet(fn, *a, **kw):
    with redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_hand_case(as_tensor):
    """One-frame gap closed in pass 2; an end taken in pass 2 that a nearer start of pass 3 cannot have; a pair dropped at 21
    pixels whose start is closed by another partner in pass 3; a gap blocked by movie_start; a gap longer than max_gap."""
    wrap = (lambda a: torch.from_numpy(np.asarray(a))) if as_tensor else (lambda a: a)
    back = (lambda a: a.numpy()) if as_tensor else (lambda a: a)
    coords, counts, ms = wrap(gc.hand_padded()), wrap(gc.HAND_COUNTS), wrap(gc.HAND_MOVIE_START)
    link = T.link_particles_movie(coords, counts, gc.HAND_MAX_DISTANCE, ms)
    assert np.array_equal(back(link), gc.HAND_LINK)
    gp, gf = T.close_gaps_movie(coords, counts, link, gc.HAND_MAX_GAP, gc.HAND_MAX_DISTANCE, ms)
    assert torch.is_tensor(gp) == as_tensor and back(gp).dtype == np.int32 and back(gf).dtype == np.int32
    assert np.array_equal(back(gp), gc.HAND_GAP_PARTNER) and np.array_equal(back(gf), gc.HAND_GAP_FRAMES)
    ids, lengths, n = T.chain_tracks(link, counts, ms, gp, gf)
    assert np.array_equal(back(ids), gc.HAND_IDS) and int(n[0]) == len(gc.HAND_LENGTHS)
    assert back(lengths)[:len(gc.HAND_LENGTHS)].tolist() == gc.HAND_LENGTHS and not back(lengths)[len(gc.HAND_LENGTHS):].any()
    # max_gap = 1 keeps the two one-frame gaps and leaves S open; without movie_start the last gap closes too
    gp1, gf1 = T.close_gaps_movie(coords, counts, link, 1, gc.HAND_MAX_DISTANCE, ms)
    assert np.array_equal(back(gf1), np.where(gc.HAND_GAP_FRAMES == 2, 2, 0))
    assert np.array_equal(back(gp1), np.where(gc.HAND_GAP_FRAMES == 2, gc.HAND_GAP_PARTNER, -1))
    link_one = T.link_particles_movie(coords, counts, gc.HAND_MAX_DISTANCE)
    gpn, gfn = T.close_gaps_movie(coords, counts, link_one, gc.HAND_MAX_GAP, gc.HAND_MAX_DISTANCE)
    assert back(gpn)[6, 0] == 3 and back(gfn)[6, 0] == 2
    # the filled rows, half-to-even included
    t = lambda a: torch.from_numpy(np.asarray(back(a)))                                        # noqa: E731
    fr, y, x, tid, in_long, filled = T.fill_gaps(t(coords), t(counts), t(ids), t(lengths), t(gp), t(gf), 1)
    assert bool(in_long.all()) and int(filled.sum()) == len(gc.HAND_FILLED)
    assert list(zip(fr[filled].tolist(), y[filled].tolist(), x[filled].tolist(), tid[filled].tolist())) == gc.HAND_FILLED
    assert len(fr) == int(gc.HAND_COUNTS.sum()) + len(gc.HAND_FILLED)
    key = fr * 100 + tid
    assert bool((key[1:] > key[:-1]).all())                      # frames ascending, ascending id within a frame, no doubles


@pytest.fixture(scope="module")
def walk():
    coords, counts = gc.walk_padded()
    ms = np.zeros(len(counts), np.uint8)
    ms[[23, 41]] = 1
    link = T.link_particles_movie(coords, counts, 15, ms)
    return coords, counts, ms, link, {k: T.close_gaps_movie(coords, counts, link, k, 15, ms) for k in gc.WALK_MAX_GAPS}


@pytest.mark.parametrize("max_gap", gc.WALK_MAX_GAPS)
def test_structure_on_a_sequence_with_dropouts(walk, max_gap):
    coords, counts, ms, link, results = walk
    gp, gf = results[max_gap]
    F, cap = link.shape
    beyond = np.arange(cap)[None, :] >= counts[:, None]
    assert (gp[beyond] == -1).all() and (gf[beyond] == 0).all()
    assert set(np.unique(gf)) <= {0} | set(range(2, max_gap + 2)) and (gf > 0).sum() > 0
    assert ((gf > 0) == (gp >= 0)).all()
    succ = np.zeros((F, cap), np.int64)                          # successors per detection, links and gap links together
    for f in range(F):
        for j in range(counts[f]):
            assert not (link[f, j] >= 0 and gf[f, j] > 0)        # at most one predecessor
            if link[f, j] >= 0:
                succ[f - 1, link[f, j]] += 1
            g = int(gf[f, j])
            if g:
                assert f - g >= 0 and 0 <= gp[f, j] < counts[f - g]
                assert not ms[f - g + 1:f + 1].any()             # no link crosses a movie_start
                d = coords[f, j].astype(np.float64) - coords[f - g, gp[f, j]]
                assert np.sqrt(d[0] * d[0] + d[1] * d[1]) <= 15
                succ[f - g, gp[f, j]] += 1
    assert succ.max() == 1
    # passes are ordered: a smaller max_gap gives the same links up to its own reach
    for smaller in gc.WALK_MAX_GAPS:
        if smaller < max_gap:
            sp, sf = results[smaller]
            keep = (gf > 0) & (gf <= smaller + 1)
            assert np.array_equal(np.where(keep, gf, 0), sf) and np.array_equal(np.where(keep, gp, -1), sp)
    # chained: every track has at most one detection per frame
    ids, lengths, n = T.chain_tracks(link, counts, ms, gp, gf)
    for f in range(F):
        assert len(set(ids[f, :counts[f]].tolist())) == counts[f]
    assert lengths[:int(n[0])].sum() == counts.sum() and np.array_equal(np.bincount(ids[ids >= 0]), lengths[:int(n[0])])
    ids0, _, n0 = T.chain_tracks(link, counts, ms)
    assert int(n[0]) == int(n0[0]) - int((gf > 0).sum())         # every gap link joins two tracks


def test_track_count_follows_from_the_planted_dark_runs():
    frames, runs, owner = gc.lattice_scene()
    coords, counts = T._padded_detections(frames, None)
    link = T.link_particles_movie(coords, counts, 15)
    particles = len(runs)
    want = {3: particles, 1: particles + int((runs >= 2).sum()), 0: particles + len(runs)}
    for max_gap, n_want in want.items():
        if max_gap:
            gp, gf = T.close_gaps_movie(coords, counts, link, max_gap, 15)
            ids, lengths, n = T.chain_tracks(link, counts, None, gp, gf)
        else:
            ids, lengths, n = T.chain_tracks(link, counts)
        assert int(n[0]) == n_want, max_gap
        owners = {}
        for f, own in enumerate(owner):
            for j, p in enumerate(own):
                owners.setdefault(int(ids[f, j]), set()).add(int(p))
        assert all(len(v) == 1 for v in owners.values())          # every track's rows belong to one particle
        if max_gap == 3:
            assert sorted(next(iter(v)) for v in owners.values()) == list(range(particles))
            assert lengths[:particles].tolist() == [gc.LATTICE_FRAMES - r for r in runs[[next(iter(owners[i])) for i in range(particles)]]]


def test_filling_gives_gap_free_tracks_that_msd_and_sequences_accept():
    frames, runs, _ = gc.lattice_scene()
    coords, counts = T._padded_detections(frames, None)
    link = T.link_particles_movie(coords, counts, 15)
    gp, gf = T.close_gaps_movie(coords, counts, link, 2, 15)                                   # the runs of 3 stay open
    ids, lengths, n = T.chain_tracks(link, counts, None, gp, gf)
    t = torch.from_numpy
    min_len = 20
    fr, y, x, tid, in_long, filled = T.fill_gaps(t(coords), t(counts), t(ids), t(lengths), t(gp), t(gf), min_len)
    # filled positions: the float64 interpolation, rounded half to even
    n_checked = 0
    for f in range(len(counts)):
        for j in range(counts[f]):
            g = int(gf[f, j])
            for k in range(1, g):
                a, b = coords[f - g, gp[f, j]].astype(np.float64), coords[f, j].astype(np.float64)
                want = np.rint(a + (b - a) * k / g).astype(np.int64)
                row = (fr == f - g + k) & filled & (y == int(want[0])) & (x == int(want[1]))
                assert int(row.sum()) == 1
                n_checked += 1
    assert int(filled.sum()) == n_checked == int((gf[gf > 0] - 1).sum()) == int(runs[runs <= 2].sum())
    long_ids = np.flatnonzero(lengths >= min_len)
    in_long_links = np.isin(ids, long_ids) & (gf > 0)
    assert int((filled & in_long).sum()) == int((gf[in_long_links] - 1).sum()) > 0
    table = {"frame": fr, "y": y, "x": x, "track_id": tid, "in_long_track": in_long, "filled": filled}
    bfr, by, bx, btid, offsets, bfilled = T.tracks_table_by_track(table)
    assert int(bfilled.sum()) == int((filled & in_long).sum()) and len(offsets) - 1 == len(long_ids)
    for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        assert bfr[a:b].tolist() == list(range(int(bfr[a]), int(bfr[a]) + b - a))               # consecutive frames
        assert len(set(btid[a:b].tolist())) == 1
    # without the column the function returns what it always returned
    plain = T.tracks_table_by_track({k: v for k, v in table.items() if k != "filled"})
    assert len(plain) == 5 and all(torch.equal(p, q) for p, q in zip(plain, (bfr, by, bx, btid, offsets)))
    msd, d, dw = MSD.track_msd(torch.stack([by, bx], dim=1).double(), offsets)
    assert msd.shape[0] == len(long_ids) and bool(torch.isfinite(d).all())
    movie = torch.zeros(len(counts), 160, 160)
    seq, seq_track, _ = T.track_sequences(movie, bfr, by, bx, offsets, 10, 7)
    assert seq.shape[1:] == (10, 7, 7) and torch.bincount(seq_track).tolist() == ((offsets[1:] - offsets[:-1]) // 10).tolist()


def test_tracking_functions_pass_max_gap_through_and_default_to_today():
    movie, truth = gc.sim_movie()
    base = _quiet(T.track_particles_flat, movie, linking="device")
    zero = _quiet(T.track_particles_flat, movie, linking="device", max_gap=0)
    assert base[0] == zero[0] and set(zero[1]) == {"frame", "y", "x", "track_id"}
    assert all(np.array_equal(base[1][k], zero[1][k]) for k in base[1]) and torch.equal(base[2], zero[2])
    dark = sum(n for _, _, n in gc.SIM_DARK)
    assert len(base[0]) == gc.SIM_PARTICLES + len(gc.SIM_DARK)               # every dark run cuts a track
    tracks, det, _ = _quiet(T.track_particles_flat, movie, linking="device", max_gap=2)
    assert len(tracks) == gc.SIM_PARTICLES and all(len(t) == gc.SIM_FRAMES for t in tracks.values())
    assert all([f for f, _, _ in t] == list(range(gc.SIM_FRAMES)) for t in tracks.values())
    assert det["filled"].dtype == bool and int(det["filled"].sum()) == dark
    assert len(det["frame"]) == len(base[1]["frame"]) + dark
    # a filled row lands on the dark truth row: with it the recall is complete, without it the dark frames are misses
    s_fill = T.score_tracking(det["frame"], det["y"], det["x"], det["track_id"], truth)
    s_base = T.score_tracking(base[1]["frame"], base[1]["y"], base[1]["x"], base[1]["track_id"], truth)
    assert float(s_fill["recall"]) == 1.0 and float(s_base["recall"]) == 1.0 - dark / (gc.SIM_PARTICLES * gc.SIM_FRAMES)
    assert sorted(s_fill["particle_id"].tolist()) == list(range(gc.SIM_PARTICLES))
    # a gap distance of its own; pandas and the files of analyze_microscopy_sequence
    tight, _, _ = _quiet(T.track_particles_flat, movie, linking="device", max_gap=2, max_gap_distance=0.0)
    assert len(tight) > gc.SIM_PARTICLES
    _, df, _ = _quiet(T.track_particles, movie, linking="device", max_gap=2)
    assert list(df.columns) == ["frame", "y", "x", "track_id", "filled"] and int(df["filled"].sum()) == dark
    tr2, df2, _ = _quiet(T.analyze_microscopy_sequence, movie, linking="device", max_gap=2)
    assert tr2 == tracks and df2.equals(df)
    _, df0, _ = _quiet(T.track_particles, movie, linking="device")
    assert list(df0.columns) == ["frame", "y", "x", "track_id"]


def test_simulator_blinks():
    args = (4, 6, 40, 48, (0.05, 0.0004), 3)
    lifetimes = [[0, 5], [2, 3], [4, 4], [1, 5]]
    props = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
    run = lambda seed, **kw: gen.simulate_movie(*args, image_props=kw.pop("props", props), lifetimes=lifetimes,      # noqa: E731
                                                generator=torch.Generator().manual_seed(seed), **kw)
    for p in (props, None):                                                  # noise-free and with every noise source
        plain, t_plain = run(3, props=p)
        none, t_none = run(3, props=p, blink=None)
        assert torch.equal(plain, none) and set(t_plain) == set(t_none) and "visible" not in t_none
        assert all(torch.equal(t_plain[k], t_none[k]) for k in t_plain)
    mask = torch.zeros(4, 6, dtype=torch.bool)
    mask[0, 2] = mask[0, 3] = mask[3, 4] = mask[1, 0] = True                  # (1, 0) lies outside particle 1's lifetime
    movie, truth = run(3, blink=mask)
    assert truth["offsets"].tolist() == t_plain["offsets"].tolist() == [0, 6, 8, 9, 14]
    amp = run(3)[1]["amp"].clone()
    amp[mask] = 0.0
    assert torch.equal(truth["amp"], amp) and bool((truth["amp"][0, 2] == 0).all()) and bool((truth["amp"][0, 1] != 0).all())
    sigma, up = gen.psf_sigma_hr(gen.DEFAULT_IMAGE_PROPS), gen.DEFAULT_IMAGE_PROPS["upsampling_factor"]
    clean = gen.render_movie(truth["pos"], amp, sigma, 40, 48, up, first=truth["first"], last=truth["last"])
    assert torch.equal(movie, (clean + 20.0).float()) and not torch.equal(movie, run(3)[0])
    assert truth["visible"].dtype == torch.bool
    assert torch.equal(truth["visible"], ~mask[truth["particle_id"], truth["frame"]])
    assert int((~truth["visible"]).sum()) == 3
    assert torch.equal(run(3, blink=mask.numpy())[0], movie)
    # the probability form: seeded, really dark, and drawn after the amplitudes (the bright frames keep their amplitude)
    a, ta = run(5, blink=0.4)
    b, tb = run(5, blink=0.4)
    assert torch.equal(a, b) and torch.equal(ta["visible"], tb["visible"]) and 0 < int((~ta["visible"]).sum()) < 14
    bright = ta["amp"] != 0
    assert torch.equal(ta["amp"][bright], run(5)[1]["amp"][bright])
    assert bool(run(5, blink=0.0)[1]["visible"].all())
    for bad in (1.0, -0.1, float("nan"), True, "0.1", mask[:3], mask.float(), mask.numpy().astype(np.uint8), mask[:, :5]):
        with pytest.raises(ValueError, match="blink"):
            run(3, blink=bad)


def test_argument_errors():
    coords, counts = gc.hand_padded(), gc.HAND_COUNTS
    for bad in (-1, 0, T.LINK_MAX_GAP + 1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="max_gap"):
            T.close_gaps_movie(coords, counts, gc.HAND_LINK, bad)
    assert T.LINK_MAX_GAP == 8
    T.close_gaps_movie(coords, counts, gc.HAND_LINK, 2.0)                    # an integral float is an integer
    with pytest.raises(ValueError, match="NaN"):
        T.close_gaps_movie(coords, counts, gc.HAND_LINK, 2, float("nan"))
    with pytest.raises(ValueError, match="link must be"):
        T.close_gaps_movie(coords, counts, gc.HAND_LINK[:3], 2)
    with pytest.raises(ValueError, match="movie_start"):
        T.close_gaps_movie(coords, counts, gc.HAND_LINK, 2, movie_start=[1, 0])
    with pytest.raises(ValueError, match="both"):
        T.chain_tracks(gc.HAND_LINK, counts, gap_partner=gc.HAND_GAP_PARTNER)
    with pytest.raises(ValueError, match="gap_partner and gap_frames must be"):
        T.chain_tracks(gc.HAND_LINK, counts, None, gc.HAND_GAP_PARTNER[:2], gc.HAND_GAP_FRAMES[:2])
    movie = np.zeros((4, 32, 32), np.float32)
    for bad in (-1, T.LINK_MAX_GAP + 1, 0.5):
        with pytest.raises(ValueError, match="max_gap"):
            T.track_particles_flat(movie, linking="device", max_gap=bad)
    with pytest.raises(ValueError, match="NaN"):
        T.track_particles_flat(movie, linking="device", max_gap=1, max_gap_distance=float("nan"))
    for fn in (T.track_particles_flat, T.track_particles, T.analyze_microscopy_sequence):
        with pytest.raises(ValueError, match='linking="device"'):
            fn(movie, linking="host", max_gap=1)
        with pytest.raises(ValueError, match='linking="device"'):
            fn(movie, max_gap=1)
    # gap links that point nowhere are ignored by the chaining, never followed
    wild_p, wild_g = np.full_like(gc.HAND_GAP_PARTNER, 3), np.full_like(gc.HAND_GAP_FRAMES, 2)
    ids, _, n = T.chain_tracks(gc.HAND_LINK, counts, gc.HAND_MOVIE_START, wild_p, wild_g)
    assert ids.max() == int(n[0]) - 1 and ids[2, 0] == 2
    far_g = np.full_like(gc.HAND_GAP_FRAMES, T.LINK_MAX_GAP + 2)
    ids2, _, n2 = T.chain_tracks(gc.HAND_LINK, counts, gc.HAND_MOVIE_START, np.zeros_like(wild_p), far_g)
    ids0, _, n0 = T.chain_tracks(gc.HAND_LINK, counts, gc.HAND_MOVIE_START)
    assert np.array_equal(ids2, ids0) and int(n2[0]) == int(n0[0])
