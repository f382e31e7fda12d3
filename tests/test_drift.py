"""CPU: the numpy restatements of csrc/drift.hip (helpers/msd._drift_frames_numpy, _drift_integrate_numpy) against the
independent oracle of tests/drift_common.py on the common set, the front end helpers/msd.estimate_drift / subtract_drift, and
generation.simulate_movie(drift=...) on the CPU path.  tests/test_drift_gpu.py holds the kernels against the restatements, bit
for bit, on the same set.

Bounds.  The median is an order statistic and (a + b) / 2 of two of the inputs: bitwise.  The mean is a sum of the same n
terms in another order, divided by n: within n 2^-52 sum|d| of the oracle's fsum / n.  The velocity and the drift are held to
the bounds that drift_common.oracle_integrate derives term by term."""
import numpy as np
import pytest
import torch

import drift_common as dc
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as msd_mod
from moleculardiffusion_mivit_amd.helpers import tracking as trk

H = dc.HALF_WINDOW


def _pairs(min_pairs=1):
    pos, frames, offsets, use = dc.common_table()
    t = lambda a: torch.from_numpy(a.copy())                                # noqa: E731
    rows, counts, fo, rej = msd_mod._drift_pairs(t(pos), t(frames), t(offsets), t(use), dc.N_FRAMES, min_pairs)
    return rows.numpy(), counts.numpy(), fo.numpy(), rej


def test_the_common_set_holds_every_frame_size_and_special_track():
    pos, frames, offsets, use = dc.common_table()
    inc, rejected = dc.oracle_increments(pos, frames, offsets, use, dc.N_FRAMES)
    assert {f: len(v) for f, v in enumerate(inc) if f in dc.FRAME_PAIRS} == dc.FRAME_PAIRS
    assert len(inc[0]) == 0 and len(inc[dc.N_FRAMES - 1]) == 0 and rejected == dc.N_REJECTED
    lengths = np.diff(offsets)
    assert {0, 1, 2, 3} <= set(lengths.tolist()) and not use.all()
    assert np.isnan(pos).any() and np.isinf(pos).any()
    for f in dc.TIE_FRAMES:
        assert sorted(repr(tuple(e)) for e in inc[f]) == sorted(repr(e) for e in dc.TIES[f])       # repr tells -0.0 from 0.0


@pytest.mark.parametrize("min_pairs", [1, 2])
def test_the_pair_list_is_the_oracles_selection(min_pairs):
    pos, frames, offsets, use = dc.common_table()
    inc, rejected = dc.oracle_increments(pos, frames, offsets, use, dc.N_FRAMES, min_pairs)
    rows, counts, fo, rej = _pairs(min_pairs)
    assert rej == rejected == dc.N_REJECTED
    assert counts.tolist() == [len(v) for v in inc] and fo.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert (counts[1] == 0) == (min_pairs == 2)                             # the frame that min_pairs = 2 empties
    for f in range(dc.N_FRAMES):
        r = rows[fo[f]:fo[f + 1]]
        assert (np.diff(r) > 0).all() and (frames[r] == f).all()
        d = pos[r] - pos[r - 1]
        assert np.array_equal(dc.bits(d), dc.bits(np.array(inc[f], dtype=np.float64).reshape(-1, 2)))


@pytest.mark.parametrize("min_pairs", [1, 2])
def test_frames_restatement_against_the_oracle(min_pairs):
    pos, frames, offsets, use = dc.common_table()
    inc, _ = dc.oracle_increments(pos, frames, offsets, use, dc.N_FRAMES, min_pairs)
    rows, counts, fo, _ = _pairs(min_pairs)
    median = msd_mod._drift_frames_numpy(pos, rows, fo, 1)
    want, _ = dc.oracle_stat(inc, "median")
    assert np.array_equal(dc.bits(median), dc.bits(np.array(want))), "the median is bitwise"
    mean = msd_mod._drift_frames_numpy(pos, rows, fo, 0)
    want, sum_abs = dc.oracle_stat(inc, "mean")
    for f in range(dc.N_FRAMES):
        for axis in range(2):
            bound = counts[f] * dc.EPS * sum_abs[f][axis]
            err = abs(mean[f, axis] - want[f][axis])
            assert err <= bound, (f, axis, err, bound)
        if counts[f] == 0:
            assert np.array_equal(dc.bits(mean[f]), dc.bits(np.zeros(2)))   # +0, not -0


# the long case runs with h = 0 and the common half window only
@pytest.mark.parametrize("F,h", [(F, h) for F in dc.INTEGRATE_F for h in (0, 1, H) if F < 1000 or h != 1])
def test_integrate_restatement_against_the_oracle(F, h):
    stat, n = dc.integrate_case(F)
    vel, drift = msd_mod._drift_integrate_numpy(stat, n, h)
    assert vel.shape == drift.shape == (F, 2)
    wv, wd, vb, db = dc.oracle_integrate(stat.tolist(), n.tolist(), h)
    wv, wd, vb, db = (np.array(a).reshape(F, 2) for a in (wv, wd, vb, db))
    assert (np.abs(vel - wv) <= vb).all(), float((np.abs(vel - wv) - vb).max())
    assert (np.abs(drift - wd) <= db).all(), float((np.abs(drift - wd) - db).max())
    assert np.array_equal(dc.bits(vel[0]), dc.bits(np.zeros(2)))
    if h == 0:                                                              # stat itself, bit for bit, not n * s / n
        assert np.array_equal(dc.bits(vel[1:]), dc.bits(stat[1:]))
    # a wider window than the movie sees every frame from 1 on
    if F <= 2 * H + 1:
        wide, _ = msd_mod._drift_integrate_numpy(stat, n, 10 * F + 5)
        allf, _ = msd_mod._drift_integrate_numpy(stat, n, F)
        assert np.array_equal(dc.bits(wide), dc.bits(allf))


def test_windows_are_cut_at_both_ends():
    """Small integers with weight 1: every window mean is one exactly rounded division, so == holds.  Frame 0 (stat 1e6 here)
    is in no window, and the last frame's window ends at the movie's end."""
    stat = np.array([[1e6, -1e6], [1, 2], [3, 5], [8, 13], [21, 34], [55, 89], [144, 233]], dtype=np.float64)
    n = np.ones(7, np.int32)
    vel, drift = msd_mod._drift_integrate_numpy(stat, n, 2)
    for f in range(1, 7):
        g0, g1 = max(1, f - 2), min(6, f + 2)
        assert vel[f].tolist() == [stat[g0:g1 + 1, a].sum() / (g1 - g0 + 1) for a in range(2)], f
    assert vel[0].tolist() == [0.0, 0.0]
    # weights: a frame without pairs does not count, a window without any gives 0
    n = np.array([5, 0, 0, 0, 2, 0, 6], np.int32)
    vel, _ = msd_mod._drift_integrate_numpy(stat, n, 1)
    assert vel[1].tolist() == [0.0, 0.0] and vel[2].tolist() == [0.0, 0.0]
    assert vel[3].tolist() == [21.0, 34.0] and vel[5].tolist() == [(2 * 21 + 6 * 144) / 8, (2 * 34 + 6 * 233) / 8]


def _rigid_table(drift, n_particles=7, seed=3):
    """Particles that do not move on a stage that does: every position is start + drift[f], all multiples of 1/8."""
    rng = np.random.default_rng(seed)
    F = len(drift)
    start = rng.integers(40, 400, (n_particles, 2)) / 8.0
    pos = (start[:, None, :] + drift[None, :, :]).reshape(-1, 2)
    frames = np.tile(np.arange(F), n_particles)
    offsets = np.arange(n_particles + 1) * F
    return pos, frames, offsets


@pytest.mark.parametrize("estimator", ["mean", "median"])
def test_a_rigid_planted_drift_is_recovered_exactly(estimator):
    rng = np.random.default_rng(5)
    steps = rng.integers(-6, 7, (300, 2)) / 8.0                             # 300 frames: two blocks of the running sum
    steps[0] = 0.0
    planted = np.cumsum(steps, axis=0)
    pos, frames, offsets = _rigid_table(planted)
    out = msd_mod.estimate_drift(pos, frames, offsets, estimator=estimator)
    assert np.array_equal(out["drift"], planted) and np.array_equal(out["velocity"], steps)
    assert out["n_pairs"].dtype == np.int32 and out["n_pairs"].tolist() == [0] + [7] * 299 and out["n_rejected"] == 0
    assert np.array_equal(msd_mod.subtract_drift(pos, frames, out["drift"]), pos - planted[frames])
    # a constant velocity survives any smoothing exactly: every window mean is n v / n
    planted = np.arange(300)[:, None] * np.array([0.375, -0.25])
    pos, frames, offsets = _rigid_table(planted)
    for h in (0, 2, H, 1000):
        out = msd_mod.estimate_drift(pos, frames, offsets, estimator=estimator, smoothing=h)
        assert np.array_equal(out["drift"], planted), h
        assert np.array_equal(out["velocity"][1:], np.tile([0.375, -0.25], (299, 1)))


def test_estimate_drift_front_end_kinds_and_arguments():
    pos, frames, offsets, use = dc.common_table()
    for estimator in ("mean", "median"):
        a = msd_mod.estimate_drift(pos, frames, offsets, n_frames=dc.N_FRAMES, estimator=estimator, smoothing=1, use=use)
        t = msd_mod.estimate_drift(*(torch.from_numpy(v.copy()) for v in (pos, frames, offsets)), n_frames=dc.N_FRAMES,
                                   estimator=estimator, smoothing=1, use=torch.from_numpy(use.copy()))
        assert set(a) == set(t) == {"drift", "velocity", "n_pairs", "n_rejected"}
        assert a["n_rejected"] == t["n_rejected"] == dc.N_REJECTED
        for k in ("drift", "velocity", "n_pairs"):
            assert isinstance(a[k], np.ndarray) and torch.is_tensor(t[k])
            assert np.array_equal(dc.bits(a[k]), dc.bits(t[k].numpy())), (estimator, k)
        assert a["drift"].shape == (dc.N_FRAMES, 2) and a["n_pairs"].dtype == np.int32 and t["n_pairs"].dtype == torch.int32
        assert np.isfinite(a["drift"]).all()
    # n_frames defaults to the last frame + 1; int32 frames and offsets are taken as well
    d = msd_mod.estimate_drift(pos, frames.astype(np.int32), offsets.astype(np.int32), use=use)
    assert d["drift"].shape == (int(frames.max()) + 1, 2)
    # without the mask the masked row's two increments come back
    e = msd_mod.estimate_drift(pos, frames, offsets)
    assert e["n_pairs"][15] == d["n_pairs"][15] + 1 and e["n_pairs"][16] == d["n_pairs"][16] + 1
    # an empty table
    z = msd_mod.estimate_drift(np.zeros((0, 2)), np.zeros(0, np.int64), np.zeros(1, np.int64))
    assert z["drift"].shape == (0, 2) and z["n_pairs"].shape == (0,)
    z = msd_mod.estimate_drift(np.zeros((0, 2)), np.zeros(0, np.int64), np.zeros(1, np.int64), n_frames=3)
    assert z["drift"].tolist() == [[0.0, 0.0]] * 3


def test_every_validation_error():
    pos, frames, offsets, use = dc.common_table()
    ok = dict(positions=pos, frames=frames, offsets=offsets)
    bad = [
        (dict(estimator="mode"), "estimator"),
        (dict(smoothing=-1), "smoothing"), (dict(smoothing=1.5), "smoothing"), (dict(smoothing=True), "smoothing"),
        (dict(min_pairs=0), "min_pairs"), (dict(min_pairs=2.5), "min_pairs"),
        (dict(positions=pos[:, :1]), r"positions must be \[N, 2\]"), (dict(positions=pos.reshape(-1)), "positions"),
        (dict(frames=frames[:-1]), "frames must be"), (dict(frames=frames.astype(np.float64)), "integers"),
        (dict(frames=frames - 1), "frames must be >= 0"),
        (dict(offsets=offsets[:-1]), "offsets"), (dict(offsets=offsets[::-1].copy()), "offsets"),
        (dict(n_frames=int(frames.max())), "n_frames"), (dict(n_frames=-1), "n_frames"), (dict(n_frames=2.5), "n_frames"),
        (dict(use=use[:-1]), "use"), (dict(use=use.astype(np.int64)), "use"),
        (dict(frames=torch.from_numpy(frames.copy())), "all be tensors or all be arrays"),
        (dict(use=torch.from_numpy(use.copy())), "all be tensors or all be arrays"),
    ]
    for change, match in bad:
        with pytest.raises(ValueError, match=match):
            msd_mod.estimate_drift(**{**ok, **change})
    drift = np.zeros((dc.N_FRAMES, 2))
    for args, match in [((pos[:, :1], frames, drift), "positions"), ((pos, frames, drift[:, :1]), "drift must be"),
                        ((pos, frames[:-1], drift), "frames must be"), ((pos, frames.astype(np.float32), drift), "integers"),
                        ((pos, frames, drift[:5]), "frames must lie in"), ((pos, frames - 1, drift), "frames must lie in"),
                        ((pos, torch.from_numpy(frames.copy()), drift), "all be tensors or all be arrays")]:
        with pytest.raises(ValueError, match=match):
            msd_mod.subtract_drift(*args)
    movie = torch.zeros(4, 16, 16)
    for d in ("mean", {"window": 3}, 1):
        with pytest.raises(ValueError, match="drift must be None or a dict"):
            trk.estimate_track_diffusion(movie, None, 4, drift=d)


def test_subtract_drift_round_trip():
    rng = np.random.default_rng(9)
    F, n = 12, 40
    drift = rng.integers(-80, 80, (F, 2)) / 8.0
    pos = rng.integers(0, 512, (n, 2)) / 8.0
    frames = rng.integers(0, F, n)
    moved = pos + drift[frames]
    assert np.array_equal(msd_mod.subtract_drift(moved, frames, drift), pos)
    back = msd_mod.subtract_drift(torch.from_numpy(moved), torch.from_numpy(frames), torch.from_numpy(drift))
    assert torch.is_tensor(back) and np.array_equal(back.numpy(), pos)
    assert msd_mod.subtract_drift(np.zeros((0, 2)), np.zeros(0, np.int64), drift).shape == (0, 2)


# ----------------------------------------------------------------------------------------------------------------------
# generation.simulate_movie(drift=...), CPU path
# ----------------------------------------------------------------------------------------------------------------------
NP_, F_, NPOS = 4, 6, 2
PROPS = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}


ABSENT = object()


def _movie(drift=ABSENT, seed=4, **kw):
    g = torch.Generator().manual_seed(seed)
    extra = {} if drift is ABSENT else {"drift": drift}
    movie, truth = gen.simulate_movie(NP_, F_, 48, 48, (0.3, 0.0), NPOS, image_props=PROPS, generator=g, **extra, **kw)
    return movie, truth, g.get_state()


def test_simulate_movie_zero_drift_changes_nothing():
    movie, truth, state = _movie()
    for zero in (np.zeros((F_, 2)), torch.zeros(F_, 2), (0.0, 0.0), None):
        m, t, s = _movie(zero)
        assert torch.equal(m, movie) and torch.equal(s, state)
        for k in ("y", "x", "pos"):
            assert np.array_equal(dc.bits(t[k].numpy().astype(np.float64)), dc.bits(truth[k].numpy().astype(np.float64))), k
        assert set(t) == set(truth) | (set() if zero is None else {"drift"})
        if zero is not None:
            assert t["drift"].dtype == torch.float64 and t["drift"].shape == (F_, 2) and not bool(t["drift"].any())


def test_simulate_movie_drift_moves_every_position_by_its_frames_offset():
    """The rounding model: truth["pos"] = float32(pos + drift[f]) with the float32 position pos of the run without drift and
    the float64 drift, rounded once; truth["y"], truth["x"] are the float64 means of those over the frame's sub-positions."""
    movie, truth, state = _movie()
    v = (0.25, -0.4)
    table = torch.arange(F_, dtype=torch.float64).view(F_, 1) * torch.tensor(v, dtype=torch.float64).view(1, 2)
    m_pair, t_pair, s_pair = _movie(v)
    m_tab, t_tab, s_tab = _movie(table.numpy())
    assert torch.equal(m_pair, m_tab) and not torch.equal(m_pair, movie)
    for k in t_pair:
        assert torch.equal(t_pair[k], t_tab[k]), k
    assert torch.equal(s_pair, state) and torch.equal(s_tab, state)        # nothing is drawn for the drift
    assert torch.equal(t_pair["drift"], table)
    want = (truth["pos"].double() + table.repeat_interleave(NPOS, dim=0).view(1, F_ * NPOS, 2)).float()
    assert torch.equal(t_pair["pos"], want)
    mean = want.double().view(NP_, F_, NPOS, 2).mean(dim=2)
    assert torch.equal(t_pair["y"], mean[t_pair["particle_id"], t_pair["frame"], 0])
    assert torch.equal(t_pair["x"], mean[t_pair["particle_id"], t_pair["frame"], 1])
    for k in ("frame", "particle_id", "offsets", "D", "amp"):
        assert torch.equal(t_pair[k], truth[k]), k
    # what estimate_drift sees in the truth table is the planted velocity, up to the particles' own motion / n
    est = msd_mod.estimate_drift(torch.stack([t_pair["y"], t_pair["x"]], 1), t_pair["frame"], t_pair["offsets"])
    still = msd_mod.estimate_drift(torch.stack([truth["y"], truth["x"]], 1), truth["frame"], truth["offsets"])
    assert torch.allclose(est["velocity"][1:] - still["velocity"][1:], torch.tensor(v, dtype=torch.float64).expand(F_ - 1, 2),
                          rtol=0, atol=1e-5)                                # float32 positions near 48: 4e-6 a rounding


def test_simulate_movie_drift_with_lifetimes_and_states_and_its_errors():
    lt = [[0, 5], [2, 4], [1, 1], [3, 5]]
    _, truth, _ = _movie(lifetimes=lt)
    _, t, _ = _movie((0.5, 0.125), lifetimes=lt)
    assert torch.equal(t["frame"], truth["frame"]) and torch.equal(t["offsets"], truth["offsets"])
    g = torch.Generator().manual_seed(2)
    _, ts = gen.simulate_movie(NP_, F_, 48, 48, None, NPOS, image_props=PROPS, generator=g, drift=(0.5, 0.0),
                               states={"Ds": (0.05, 0.5), "M": [[0.9, 0.1], [0.1, 0.9]]})
    assert "drift" in ts and "state" in ts
    for bad in (np.zeros((F_ + 1, 2)), np.zeros((F_, 3)), (1.0, 2.0, 3.0), 0.5, np.zeros((F_, 2), bool),
                np.zeros((F_, 2), np.complex128), "fast", (float("nan"), 0.0), np.full((F_, 2), np.inf)):
        with pytest.raises(ValueError, match="drift must be"):
            _movie(bad)
