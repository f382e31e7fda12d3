"""CPU: the numpy restatement of csrc/directed_ml.hip (helpers/msd.estimate_directed_ml, directed_loglik) against the dense
statement of the likelihood (directed_ml_common.dense_fit), against estimate_diffusion_ml at velocity 0, against a scalar
polish of the dense profile cost, under a velocity added to the tracks, and on tracks drawn by a construction that does not
use the model's covariance; the statuses, the argument handling, and the simulator's velocity options
(generation.directed_single_state, simulate_movie(velocity=)).  tests/test_directed_ml_gpu.py holds the kernels against the
restatement."""
import os

import numpy as np
import pytest
import torch
from scipy.optimize import minimize_scalar

import directed_ml_common as dc
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as M

R = dc.R_FRAME
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment", "simulate_movie_before_states.npz")
PROPS = {"particle_intensity": [500, 20], "background_intensity": [100, 10], "poisson_noise": 100}
KEYS = {"D_dir", "D_dir_std", "velocity", "velocity_std", "speed", "speed_std", "loglik", "lr_brownian", "p_brownian",
        "n_increments", "status"}
CHI2_2_95 = 5.991


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


# ----------------------------------------------------------------------------------------------------------------------
# against the dense statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blur", [0.0, 1.0 / 6.0])
@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("rows", [3, 4, 9, 31, 60])
def test_loglik_and_profiled_velocity_against_the_dense_statement(rows, gaps, blur):
    rng = np.random.default_rng(100 * rows + 10 * gaps + int(blur > 0))
    vel = rng.normal(0.0, 1.0, (3, 2))
    pos, var, fr, off = dc.draw(rng, 3, rows, 0.3, 0.02, vel, 0.5, frames=2 * rows if gaps else None)
    var[rows + 1, 0] = 0.0                                                 # one zero variance
    D = np.array([0.1, 0.3, 0.9])
    prof = M.directed_loglik(pos, off, D, None, var, fr, dt=0.5, blur=blur)
    given = M.directed_loglik(pos, off, D, vel + 0.1, var, fr, dt=0.5, blur=blur)
    assert set(prof) == {"loglik", "velocity", "velocity_std"} and set(given) == {"loglik"}
    worst = 0.0
    for k in range(3):
        X, v, f = pos[off[k]:off[k + 1]], var[off[k]:off[k + 1]], fr[off[k]:off[k + 1]]
        ll, u, sd = dc.dense_fit(X, v, f, D[k], 0.5, blur)
        llg, _, _ = dc.dense_fit(X, v, f, D[k], 0.5, blur, vel[k] + 0.1)
        errs = (abs(prof["loglik"][k] - ll) / abs(ll), abs(given["loglik"][k] - llg) / abs(llg),
                np.abs(prof["velocity"][k] - u).max() / sd.min(), np.abs(prof["velocity_std"][k] / sd - 1.0).max())
        worst = max(worst, *errs)
    print(f"rows {rows}, gaps {gaps}, R {blur:.3f}: worst difference to the dense statement {worst:.3g} (bar {dc.LOGLIK_BAR:g})")
    assert worst <= dc.LOGLIK_BAR


def test_velocity_zero_is_the_likelihood_of_free_diffusion():
    rng = np.random.default_rng(11)
    pos, var, fr, off = dc.draw(rng, 12, 40, 0.2, 0.02, (0.3, -0.2), 0.5, frames=55)
    free = M.estimate_diffusion_ml(pos, off, var, fr, dt=0.5, blur=R)
    assert (free["status"] == 0).all()
    at = M.directed_loglik(pos, off, free["D_ml"], (0.0, 0.0), var, fr, dt=0.5, blur=R)["loglik"]
    rel = np.abs(at - free["loglik"]) / np.abs(free["loglik"])
    print(f"velocity 0 against estimate_diffusion_ml at the same D: worst relative difference {rel.max():.3g} (bar 1e-12)")
    assert (rel <= 1e-12).all()


def test_the_search_against_a_polish():
    """scipy's bounded scalar minimiser on the dense profile cost in ln D, about the restatement's answer"""
    rng = np.random.default_rng(12)
    parts = [dc.draw(rng, 8, rows, D, 0.02, rng.normal(0.0, 1.0, (8, 2)), 0.5, frames=frames)
             for rows, D, frames in ((12, 0.05, None), (30, 0.5, 45), (60, 0.2, None))]
    pos, var, fr = (np.concatenate([p[i] for p in parts]) for i in range(3))
    off = np.concatenate([[0], np.cumsum([rows for rows in (12, 30, 60) for _ in range(8)])])
    fit = M.estimate_directed_ml(pos, off, var, fr, dt=0.5, blur=R)
    fine = np.nonzero(fit["status"] == 0)[0]
    assert len(fine) >= 20
    worst = -np.inf
    for k in fine:
        X, v, f = pos[off[k]:off[k + 1]], var[off[k]:off[k + 1]], fr[off[k]:off[k + 1]]
        cost = lambda u: -2.0 * dc.dense_fit(X, v, f, np.exp(u), 0.5, R)[0]     # noqa: E731
        u0 = np.log(fit["D_dir"][k])
        best = minimize_scalar(cost, bounds=(u0 - 1.0, u0 + 1.0), method="bounded", options={"xatol": 1e-10})
        worst = max(worst, cost(u0) - min(best.fun, cost(u0)))
    print(f"{len(fine)} status-0 tracks: the search loses at most {worst:.3g} in -2 log L to the polish (bar {dc.SEARCH_LOSS_BAR:g})")
    assert worst <= dc.SEARCH_LOSS_BAR


def test_what_the_D_bar_lets_the_velocity_move_by():
    """the measurement behind directed_ml_common.BARS["velocity"] and ["velocity_std"]"""
    b = dc.batch()
    args = (b["pos"], b["var"], b["frames"].astype(np.int64), b["use"], b["offsets"], dc.BATCH_DT, dc.BATCH_R)
    fit = dict(zip(M._DM_OUTS, M._directed_ml_numpy(*args)))
    fine = fit["status"] == 0
    assert fine.sum() >= dc.MIN_STATUS_0
    _, v0, s0 = M._directed_loglik_numpy(*args, fit["D_dir"], None)
    _, v1, s1 = M._directed_loglik_numpy(*args, fit["D_dir"] * np.exp(dc.BARS["D"]), None)
    assert np.array_equal(v0[fine], fit["velocity"][fine]) and np.array_equal(s0[fine], fit["velocity_std"][fine])
    moved = {"velocity": float((np.abs(v1 - v0)[fine] / s0[fine]).max()), "velocity_std": float(np.abs(s1 / s0 - 1.0)[fine].max())}
    print("what D e^{1e-6} moves:", moved, "recorded:", dc.MOVED_BY_THE_D_BAR)
    for k, m in moved.items():
        assert 0.9 * dc.MOVED_BY_THE_D_BAR[k] <= m <= dc.MOVED_BY_THE_D_BAR[k] and dc.BARS[k] == 10.0 * dc.MOVED_BY_THE_D_BAR[k]


def test_a_velocity_added_to_the_tracks_is_added_to_the_estimate():
    """positions reach 1e4 step standard deviations; it fails where D_ref or the sums contain the velocity"""
    rng = np.random.default_rng(13)
    dt, D = 0.5, 0.5
    pos, var, fr, off = dc.draw(rng, 30, 100, D, 0.02, (0.0, 0.0), dt, frames=130)
    base = M.estimate_directed_ml(pos, off, var, fr, dt=dt, blur=R)
    v = 1e4 * np.sqrt(2.0 * D * dt) / (129 * dt) * np.array([0.6, -0.8])
    moved = M.estimate_directed_ml(pos + v[None, :] * (fr[:, None] * dt), off, var, fr, dt=dt, blur=R)
    dv = np.abs((moved["velocity"] - base["velocity"]) - v[None, :]) / base["velocity_std"]
    dD = np.abs(moved["D_dir"] / base["D_dir"] - 1.0)
    print(f"velocity changes by v to within {dv.max():.3g} of velocity_std (bar 1e-5), D_dir stays within {dD.max():.3g} (bar {dc.BARS['D']:g})")
    assert (base["status"] == 0).all() and np.array_equal(moved["status"], base["status"])
    assert (dv <= 1e-5).all() and (dD <= dc.BARS["D"]).all()


# ----------------------------------------------------------------------------------------------------------------------
# statistics with fixed seeds: 200 tracks of 100 rows, D = 0.5, dt = 0.5, v0 = 0.02
# ----------------------------------------------------------------------------------------------------------------------
STAT = dict(n=200, rows=100, D=0.5, dt=0.5, v0=0.02)


def _stat_fit(seed, velocity):
    pos, var, fr, off = dc.draw(np.random.default_rng(seed), STAT["n"], STAT["rows"], STAT["D"], STAT["v0"], velocity, STAT["dt"])
    return M.estimate_directed_ml(pos, off, var, fr, dt=STAT["dt"], blur=R)


def test_statistics_on_directed_tracks():
    v = np.array([0.6, -0.4])
    fit = _stat_fit(21, v)
    assert (fit["status"] == 0).all() and (fit["n_increments"] == 99).all()
    pull_v = _rms((fit["velocity"] - v[None, :]) / fit["velocity_std"])
    pull_d = _rms((np.log(fit["D_dir"]) - np.log(STAT["D"])) / (fit["D_dir_std"] / fit["D_dir"]))
    mean_pull_d = float(np.mean((np.log(fit["D_dir"]) - np.log(STAT["D"])) / (fit["D_dir_std"] / fit["D_dir"])))
    n_found = int((fit["lr_brownian"] > CHI2_2_95).sum())
    print(f"RMS pull of the 400 velocity components {pull_v:.3f} (band [0.85, 1.15]); RMS pull of ln D_dir {pull_d:.3f} (band "
          f"[0.85, 1.30]; its mean {mean_pull_d:.3f}); lr_brownian > {CHI2_2_95}: {n_found} of 200 (at least 190), mean lr "
          f"{fit['lr_brownian'].mean():.2f}; mean speed {fit['speed'].mean():.4f} (true {np.hypot(*v):.4f}), mean speed_std "
          f"{fit['speed_std'].mean():.4f}")
    assert 0.85 <= pull_v <= 1.15
    assert 0.85 <= pull_d <= 1.30
    assert n_found >= 190
    assert ((fit["p_brownian"] < 0.05) == (fit["lr_brownian"] > -2.0 * np.log(0.05))).all()


def test_free_walks_are_not_taken_for_directed():
    fit = _stat_fit(21, (0.0, 0.0))
    lr = fit["lr_brownian"]
    frac = float((lr > CHI2_2_95).mean())
    print(f"free walks: least lr_brownian {lr.min():.3g} (at least -1e-6), mean {lr.mean():.3f} (band [1.5, 2.5]), fraction above "
          f"{CHI2_2_95}: {frac:.3f} (at most 0.10)")
    assert (fit["status"] == 0).all()
    assert (lr >= -1e-6).all()
    assert 1.5 <= lr.mean() <= 2.5
    assert frac <= 0.10
    assert np.array_equal(fit["p_brownian"], np.exp(-0.5 * np.maximum(lr, 0.0)))


# ----------------------------------------------------------------------------------------------------------------------
# the statuses, rows left out
# ----------------------------------------------------------------------------------------------------------------------
def _line(rows, dt=0.5):
    f = np.arange(rows, dtype=np.int64)
    return np.array([[20.0, 30.0]]) + dc.LINE_VELOCITY[None, :] * (f[:, None] * dt), f


def test_status_1_a_short_range():
    pos, _ = _line(4)
    fit = M.estimate_directed_ml(pos, np.array([0, 0, 1, 3, 4]), 0.01, dt=0.5)
    assert fit["status"].tolist() == [1, 1, 1, 1] and fit["n_increments"].tolist() == [0, 0, 1, 0]
    for k in KEYS - {"status", "n_increments"}:
        assert np.isnan(fit[k]).all(), k


def test_status_2_a_straight_line():
    """within its stated noise the velocity and its error bar stand; with no noise at all the likelihood at D = 0 does not
    exist, and neither do they"""
    pos, f = _line(40)
    pos[1::2] += 0.05
    fit = M.estimate_directed_ml(pos, np.array([0, 40]), 0.05, f, dt=0.5, blur=R)
    assert fit["status"][0] == 2 and fit["D_dir"][0] == 0.0 and np.isnan(fit["D_dir_std"][0])
    assert np.isfinite(fit["loglik"][0]) and (np.abs(fit["velocity"][0] - dc.LINE_VELOCITY) < 3.0 * fit["velocity_std"][0]).all()
    assert (fit["velocity_std"][0] > 0).all() and abs(fit["speed"][0] - np.hypot(*dc.LINE_VELOCITY)) < 3.0 * fit["speed_std"][0]
    exact, f = _line(12)
    fit = M.estimate_directed_ml(exact, np.array([0, 12]), None, f, dt=0.5)
    assert fit["status"][0] == 2 and fit["D_dir"][0] == 0.0 and fit["loglik"][0] == -np.inf
    assert np.isnan(fit["velocity"]).all() and np.isnan(fit["velocity_std"]).all()
    assert fit["lr_brownian"][0] == -np.inf and fit["p_brownian"][0] == 1.0


def test_status_3_alternating_rows_under_full_blur():
    """rows that alternate about a line, no stated noise, blur 1/4: the model's neighbouring increments are positively
    correlated and the data's negatively, so the likelihood still rises at the upper end of the bracket, 16 D_ref"""
    f = np.arange(30, dtype=np.int64)
    pos = np.array([[20.0, 30.0]]) + 0.5 * f[:, None] + np.where(f % 2 == 0, 1.0, -1.0)[:, None] * np.array([[1.0, 0.5]])
    fit = M.estimate_directed_ml(pos, np.array([0, 30]), None, f, dt=1.0, blur=0.25)
    u0 = (pos[-1] - pos[0]) / 29.0
    res = np.diff(pos, axis=0) - u0[None, :]
    d_ref = (res * res).sum() / (4.0 * 29.0)
    print("status", fit["status"][0], "D_dir / D_ref", fit["D_dir"][0] / d_ref)
    assert fit["status"][0] == 3 and abs(fit["D_dir"][0] / (16.0 * d_ref) - 1.0) < 1e-12
    assert np.isfinite(fit["velocity"]).all() and np.isfinite(fit["D_dir_std"][0])


def test_status_4_the_rule(monkeypatch):
    """Status 4 (an interior minimum whose second difference over h = 1/64 is not positive) is not reached by rows we could
    construct: for every D > 0 the covariance is positive definite whenever it is at any D, so no neighbour of an accepted D
    is rejected, and the information in ln D times h^2 is far above the cost's rounding wherever the minimum is interior.
    The rule itself is held here with the curvature replaced: the estimates stand, D_dir_std is NaN, the status is 4."""
    rng = np.random.default_rng(14)
    pos, var, fr, off = dc.draw(rng, 2, 20, 0.3, 0.02, (0.5, 0.25), 0.5)
    want = M.estimate_directed_ml(pos, off, var, fr, dt=0.5, blur=R)
    assert (want["status"] == 0).all()
    monkeypatch.setattr(M, "_ml_curvature", lambda cp, c0, cm: np.zeros_like(c0))
    got = M.estimate_directed_ml(pos, off, var, fr, dt=0.5, blur=R)
    assert (got["status"] == 4).all() and np.isnan(got["D_dir_std"]).all()
    for k in ("D_dir", "velocity", "velocity_std", "loglik", "n_increments"):
        assert np.array_equal(got[k], want[k]), k


def test_a_dropped_row_is_a_gap():
    rng = np.random.default_rng(15)
    pos, var, fr, off = dc.draw(rng, 2, 30, 0.3, 0.02, (0.5, 0.25), 0.5)
    use = np.ones(60, bool)
    use[[4, 5, 17, 40]] = False
    bad_pos, bad_var = pos.copy(), var.copy()
    bad_pos[4, 0], bad_pos[5, 1], bad_var[17, 0], bad_var[40, 1] = np.nan, np.inf, -1.0, np.inf
    off_short = np.array([0, 27, 56])
    want = M.estimate_directed_ml(pos[use], off_short, var[use], fr[use], dt=0.5, blur=R)
    assert (want["status"] == 0).all()
    for got in (M.estimate_directed_ml(pos, off, var, fr, use, dt=0.5, blur=R), M.estimate_directed_ml(bad_pos, off, bad_var, fr, dt=0.5, blur=R)):
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), k
    got = M.directed_loglik(bad_pos, off, 0.4, None, bad_var, fr, dt=0.5, blur=R)
    want = M.directed_loglik(pos[use], off_short, 0.4, None, var[use], fr[use], dt=0.5, blur=R)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ----------------------------------------------------------------------------------------------------------------------
# arguments
# ----------------------------------------------------------------------------------------------------------------------
def test_omitted_arguments_are_their_defaults_and_kinds():
    rng = np.random.default_rng(16)
    pos, var, fr, off = dc.draw(rng, 3, 20, 0.3, 0.02, (0.5, 0.25), 1.0)
    base = M.estimate_directed_ml(pos, off)
    full = M.estimate_directed_ml(pos, off, np.zeros((60, 2)), np.tile(np.arange(20), 3), np.ones(60, bool), 1.0, 0.0)
    assert set(base) == KEYS
    for k in base:
        assert np.array_equal(base[k], full[k], equal_nan=True), k
    assert base["status"].dtype == base["n_increments"].dtype == np.int64
    assert base["velocity"].shape == base["velocity_std"].shape == (3, 2) and base["speed"].shape == base["speed_std"].shape == (3,)
    v, s = base["velocity"], base["velocity_std"]
    assert np.array_equal(base["speed"], np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]))
    assert np.allclose(base["speed_std"], np.sqrt((v * v * s * s).sum(1)) / base["speed"], rtol=1e-14)
    free = M.estimate_diffusion_ml(pos, off)
    assert np.array_equal(base["lr_brownian"], 2.0 * (base["loglik"] - free["loglik"]))
    per_row, scalar = M.estimate_directed_ml(pos, off, var[:, 0]), M.estimate_directed_ml(pos, off, 0.02)
    assert np.array_equal(per_row["loglik"], M.estimate_directed_ml(pos, off, np.stack([var[:, 0]] * 2, 1))["loglik"])
    assert np.array_equal(scalar["loglik"], M.estimate_directed_ml(pos, off, np.full((60, 2), 0.02))["loglik"])
    t = M.estimate_directed_ml(torch.from_numpy(pos), torch.from_numpy(off), torch.from_numpy(var), blur=R)
    want = M.estimate_directed_ml(pos, off, var, blur=R)
    for k in want:
        assert torch.is_tensor(t[k]) and np.array_equal(t[k].numpy(), want[k], equal_nan=True), k
    tl = M.directed_loglik(torch.from_numpy(pos), torch.from_numpy(off), 0.4, torch.tensor([1.0, 2.0]))
    assert set(tl) == {"loglik"} and torch.is_tensor(tl["loglik"])
    assert np.array_equal(tl["loglik"].numpy(), M.directed_loglik(pos, off, np.full(3, 0.4), np.tile([1.0, 2.0], (3, 1)))["loglik"])
    tp = M.directed_loglik(torch.from_numpy(pos), torch.from_numpy(off), torch.full((3,), 0.4, dtype=torch.float64))
    assert all(torch.is_tensor(tp[k]) for k in ("loglik", "velocity", "velocity_std")) and tp["velocity"].shape == (3, 2)
    empty = M.estimate_directed_ml(np.zeros((0, 2)), np.zeros(1, np.int64))
    assert set(empty) == KEYS and all(len(v) == 0 for v in empty.values())
    # D negative or not finite, a velocity that is not finite, a range without an increment: NaN; D = 0 with noise is a likelihood
    ll = M.directed_loglik(pos, off, np.array([-1.0, np.inf, np.nan]))
    assert np.isnan(ll["loglik"]).all() and np.isnan(ll["velocity"]).all() and np.isnan(ll["velocity_std"]).all()
    assert np.isnan(M.directed_loglik(pos, off, 0.4, np.array([np.nan, 0.0]))["loglik"]).all()
    assert np.isnan(M.directed_loglik(pos[:1], np.array([0, 1]), 0.4)["loglik"][0])
    assert np.isfinite(M.directed_loglik(pos, off, 0.0, None, 0.02)["loglik"]).all()
    assert (M.directed_loglik(pos, off, 0.0)["loglik"] == -np.inf).all()


def test_argument_errors():
    pos, off = np.zeros((10, 2)), np.array([0, 10])
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="dt"):
            M.estimate_directed_ml(pos, off, dt=dt)
        with pytest.raises(ValueError, match="dt"):
            M.directed_loglik(pos, off, 1.0, dt=dt)
    for blur in (-0.01, 0.26, float("nan")):
        with pytest.raises(ValueError, match="blur"):
            M.estimate_directed_ml(pos, off, blur=blur)
        with pytest.raises(ValueError, match="blur"):
            M.directed_loglik(pos, off, 1.0, blur=blur)
    with pytest.raises(ValueError, match="positions"):
        M.estimate_directed_ml(np.zeros((10, 3)), off)
    with pytest.raises(ValueError, match="variances"):
        M.estimate_directed_ml(pos, off, np.zeros((9, 2)))
    with pytest.raises(ValueError, match="variance"):
        M.estimate_directed_ml(pos, off, -1.0)
    with pytest.raises(ValueError, match="use"):
        M.estimate_directed_ml(pos, off, use=np.ones(10))
    with pytest.raises(ValueError, match="frames"):
        M.estimate_directed_ml(pos, off, frames=np.zeros(10, np.int64))
    with pytest.raises(ValueError, match="tensors or all"):
        M.estimate_directed_ml(pos, torch.tensor([0, 10]))
    with pytest.raises(ValueError, match="D must"):
        M.directed_loglik(pos, off, np.ones(2))
    with pytest.raises(ValueError, match="velocity must"):
        M.directed_loglik(pos, off, 1.0, np.ones(3))


# ----------------------------------------------------------------------------------------------------------------------
# the simulator
# ----------------------------------------------------------------------------------------------------------------------
def test_directed_single_state():
    free, labels = gen.brownian_single_state(50, 30, (0.4, 0.01), dt=0.5, generator=torch.Generator().manual_seed(3))
    for zero in ((0.0, 0.0), np.zeros((50, 2))):
        still, same_labels = gen.directed_single_state(50, 30, (0.4, 0.01), zero, 0.5, generator=torch.Generator().manual_seed(3))
        assert still.dtype == free.dtype and torch.equal(still, free) and torch.equal(same_labels, labels)
    vel = torch.linspace(-1.0, 1.0, 100, dtype=torch.float64).view(50, 2)
    moved, _ = gen.directed_single_state(50, 30, (0.4, 0.01), vel, 0.5, generator=torch.Generator().manual_seed(3))
    t = torch.arange(30, dtype=torch.float64).view(30, 1, 1) * 0.5
    assert torch.equal(moved, (free.double() + t * vel.view(1, 50, 2)).float())
    for bad in ((1.0, 2.0, 3.0), np.zeros((49, 2)), (float("nan"), 0.0), "fast"):
        with pytest.raises(ValueError, match="velocity"):
            gen.directed_single_state(50, 30, (0.4, 0.0), bad)


def test_simulate_movie_without_velocity_is_unchanged():
    """the movie and the truth recorded before simulate_movie had states (tests/golden/segment), bit for bit: without the
    keyword, with None and with a zero velocity"""
    want = np.load(GOLDEN)
    for kw in ({}, {"velocity": None}, {"velocity": (0.0, 0.0)}, {"velocity": np.zeros((3, 2))}):
        g = torch.Generator().manual_seed(123)
        vid, truth = gen.simulate_movie(3, 6, 24, 24, (0.5, 0.1), 4, PROPS, generator=g, lifetimes=[[0, 5], [1, 4], [2, 5]], **kw)
        assert np.array_equal(vid.numpy(), want["movie"])
        for k in ("frame", "y", "x", "particle_id", "offsets", "D", "pos", "amp"):
            assert np.array_equal(truth[k].numpy(), want[k]), k
        assert ("velocity" in truth) == (kw.get("velocity") is not None)


def test_simulate_movie_with_velocity():
    vel = np.array([[0.5, -0.25], [0.0, 0.75], [-0.125, 0.0], [1.0, 1.0]])
    args = (4, 10, 64, 64, 0.3, 4, PROPS)
    for extra in ({}, {"alphas": 0.8}, {"states": {"Ds": [0.1, 1.0], "M": [[0.9, 0.1], [0.1, 0.9]]}}):
        a = args[:4] + (None,) + args[5:] if "states" in extra else args
        vid0, base = gen.simulate_movie(*a, generator=torch.Generator().manual_seed(7), **extra)
        vid, truth = gen.simulate_movie(*a, generator=torch.Generator().manual_seed(7), velocity=vel, **extra)
        assert truth["velocity"].dtype == torch.float64 and np.array_equal(truth["velocity"].numpy(), vel)
        assert set(truth) == set(base) | {"velocity"}
        sub = torch.arange(40, dtype=torch.float64).view(1, 40, 1) / 4.0
        assert torch.equal(truth["pos"], (base["pos"].double() + torch.from_numpy(vel).view(4, 1, 2) * sub).float())
        assert torch.equal(truth["amp"], base["amp"]) and not torch.equal(vid, vid0)
        # per frame: the mean of the moved sub-positions = the mean of the others + velocity * (frame + 3/8), to float32 rounding
        step = torch.from_numpy(vel)[truth["particle_id"]] * (truth["frame"].double() + 0.375).view(-1, 1)
        moved = torch.stack([truth["y"] - base["y"], truth["x"] - base["x"]], dim=1)
        assert float((moved - step).abs().max()) < 64 * 2.0 ** -23
    one = gen.simulate_movie(*args, generator=torch.Generator().manual_seed(7), velocity=(0.5, -0.25))[1]
    assert np.array_equal(one["velocity"].numpy(), np.tile([0.5, -0.25], (4, 1)))
    from moleculardiffusion_mivit_amd.helpers import geometry as geo
    line = geo.Geometry([geo.Edge((10.0, 10.0), (50.0, 50.0))])
    for kw in ({"geometry": line}, {"confinement": {"radius": 2.0}}):
        with pytest.raises(ValueError, match="velocity"):
            gen.simulate_movie(*args, velocity=(0.5, 0.0), **kw)
    for bad in ((1.0, 2.0, 3.0), np.zeros((3, 2)), (float("inf"), 0.0)):
        with pytest.raises(ValueError, match="velocity"):
            gen.simulate_movie(*args, velocity=bad)
