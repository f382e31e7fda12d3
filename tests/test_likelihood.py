"""CPU: helpers/msd.estimate_diffusion_ml on numpy arrays, i.e. the numpy restatement of csrc/likelihood.hip
(helpers/msd._diffusion_ml_numpy), which tests/test_likelihood_gpu.py holds the kernel against.

  dense       the likelihood it reports is the dense fp64 one (slogdet and solve on the tridiagonal covariance) at the D it
              returns, to 1e-10 relative, and no point of a 2 001-point scan of log2(D / D_ref) over [-20, 4] has a likelihood
              that is higher by more than 1e-9 of its magnitude;
  statistics  on tracks drawn from the model (tests/likelihood_common.draw: the time average of a Brownian path plus noise of
              known variance, no covariance matrix involved) it is unbiased, its error bar is right, it beats D_cve and it
              gains from knowing each row's variance; the bounds are the issue's, from a numpy prototype of 400 tracks a case;
  edges       short and empty ranges, unusable rows, a track that does not move, omitted arguments;
  arguments   every rejection is a ValueError."""
import numpy as np
import pytest
import torch

import likelihood_common as lc
from moleculardiffusion_mivit_amd.helpers import msd as M
from moleculardiffusion_mivit_amd.helpers import tracking as T

R = lc.R_FRAME


# ----------------------------------------------------------------------------------------------------------------------
# dense
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_tracks():
    """tracks of 3, 7 and 40 rows spread over 5, 12 and 55 frames, with unequal variances -> (inputs, the fit)"""
    rng = np.random.default_rng(7)
    parts = [lc.draw(rng, 1, rows, 0.08, 0.02, 0.7, frames) for rows, frames in ((3, 5), (7, 12), (40, 55))]
    pos, var, fr = (np.concatenate([p[i] for p in parts]) for i in range(3))
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])])
    return (pos, var, fr, off), M.estimate_diffusion_ml(pos, off, var, frames=fr, dt=0.7, blur=R)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_against_the_dense_likelihood(dense_tracks, k):
    (pos, var, fr, off), fit = dense_tracks
    a, b = off[k], off[k + 1]
    X, v, f = pos[a:b], var[a:b], fr[a:b]
    assert np.diff(f).max() > 1 and len(np.unique(v)) > 1, "the case has gaps and unequal variances"
    assert fit["status"][k] == 0 and fit["n_increments"][k] == b - a - 1
    D, ll = fit["D_ml"][k], fit["loglik"][k]
    want = lc.dense_loglik(X, v, f, D, 0.7, R)
    print(f"{b - a} rows: D_ml {D:.6g} +- {fit['D_ml_std'][k]:.3g}, loglik {ll:.12g}, dense {want:.12g}")
    assert abs(ll - want) <= 1e-10 * abs(want)
    scan = lc.d_ref(X, f, 0.7) * np.exp2(np.linspace(-20.0, 4.0, 2001))
    best = max(lc.dense_loglik(X, v, f, Ds, 0.7, R) for Ds in scan)
    print(f"the best of the scan lies {best - ll:.3g} above it")
    assert best <= ll + 1e-9 * abs(ll)


def test_the_error_bar_is_the_curvature_of_the_dense_likelihood(dense_tracks):
    """D_ml_std = D / sqrt(I), I the second difference of the dense log L in ln D with the step of the header, h = 1 / 64"""
    (pos, var, fr, off), fit = dense_tracks
    X, v, f, D = pos[off[2]:], var[off[2]:], fr[off[2]:], fit["D_ml"][2]
    l0, lp, lm = (lc.dense_loglik(X, v, f, D * np.exp(s / 64.0), 0.7, R) for s in (0, 1, -1))
    info = -((lp - l0) + (lm - l0)) * 4096.0
    # I h^2 is a second difference of numbers of size |log L|.  Grant each of them an error of 1e-13 |log L| (40 x 40 dense
    # algebra; the recurrence is better): four of them in I h^2 on either side, and the std takes half the relative error of I
    bound = 2 * (4 * 1e-13 * abs(l0)) / (info / 4096.0) / 2
    got = fit["D_ml_std"][2] / (D / np.sqrt(info)) - 1.0
    print(f"D_ml_std against the dense curvature: {got:.3g} (bound {bound:.3g})")
    assert abs(got) < bound


# ----------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------
def _rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


@pytest.fixture(scope="module")
def dense_case():
    """the first row of the issue's table: 400 tracks of 100 rows, D = 0.01, v0 = 0.04, mixed variances"""
    pos, var, fr, off = lc.draw(np.random.default_rng(1), 400, 100, 0.01, 0.04)
    return pos, var, off, M.estimate_diffusion_ml(pos, off, var, blur=R)


def test_unbiased_with_an_honest_error_bar(dense_case):
    pos, var, off, fit = dense_case
    D, sd = fit["D_ml"], fit["D_ml_std"]
    assert (fit["status"] == 0).all() and (fit["n_increments"] == 99).all()
    pull = _rms((D - 0.01) / sd)
    print(f"mean D_ml {D.mean():.5f} (true 0.01), RMS error {_rms(D - 0.01):.5f}, RMS pull {pull:.3f}")
    assert abs(D.mean() - 0.01) <= 0.05 * 0.01
    assert 0.85 <= pull <= 1.30


def test_tighter_than_the_covariance_estimator(dense_case):
    pos, var, off, fit = dense_case
    d_cve = M._segment_stats_numpy(pos, off, off[1:], 1.0, R)[0]
    e_ml, e_cve = _rms(fit["D_ml"] - 0.01), _rms(d_cve - 0.01)
    print(f"RMS error: D_ml {e_ml:.5f}, D_cve {e_cve:.5f}, ratio {e_ml / e_cve:.3f}")
    assert e_ml <= 0.6 * e_cve


def test_gains_from_each_rows_own_variance(dense_case):
    pos, var, off, fit = dense_case
    mean_var = np.repeat(var.reshape(400, 100, 2).mean(axis=(1, 2)), 100)
    flat = M.estimate_diffusion_ml(pos, off, mean_var, blur=R)
    assert (flat["status"] == 0).all()
    e_ml, e_flat = _rms(fit["D_ml"] - 0.01), _rms(flat["D_ml"] - 0.01)
    print(f"RMS error: with each row's variance {e_ml:.5f}, with the track's mean {e_flat:.5f}, ratio {e_ml / e_flat:.3f}")
    assert e_ml < e_flat


def test_unbiased_on_tracks_with_gaps():
    """the third row of the table: 50 observed rows spread over 70 frames, D = 0.05, v0 = 0.02"""
    pos, var, fr, off = lc.draw(np.random.default_rng(3), 400, 50, 0.05, 0.02, frames=70)
    fit = M.estimate_diffusion_ml(pos, off, var, frames=fr, blur=R)
    D, sd = fit["D_ml"], fit["D_ml_std"]
    assert (fit["status"] == 0).all()
    pull = _rms((D - 0.05) / sd)
    print(f"mean D_ml {D.mean():.5f} (true 0.05), RMS error {_rms(D - 0.05):.5f}, RMS pull {pull:.3f}")
    assert abs(D.mean() - 0.05) <= 0.05 * 0.05
    assert 0.85 <= pull <= 1.30


# ----------------------------------------------------------------------------------------------------------------------
# edges
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_batch():
    b = lc.batch()
    fit = M.estimate_diffusion_ml(b["pos"], b["offsets"], b["var"], frames=b["frames"], use=b["use"], dt=lc.BATCH_DT, blur=lc.BATCH_R)
    return b, {name: {k: v[i] for k, v in fit.items()} for i, name in enumerate(b["names"])}


def test_short_and_unusable_ranges(edge_batch):
    b, fit = edge_batch
    assert len(b["names"]) == lc.BATCH_N == len(set(b["names"]))
    for name, n_inc in (("0 rows", 0), ("1 rows", 0), ("2 rows", 1), ("every row unusable", 0), ("one usable row", 0),
                        ("3 rows, NaN in the middle", 1)):
        got = fit[name]
        assert got["status"] == 1 and got["n_increments"] == n_inc, name
        assert np.isnan(got["D_ml"]) and np.isnan(got["D_ml_std"]) and np.isnan(got["loglik"]), name
    assert fit["3 rows"]["n_increments"] == 2 and fit["3 rows"]["status"] in (0, 2)
    # a row that cannot be used is a gap: 12 rows, one of them out
    for name in ("NaN position", "inf position", "negative variance", "NaN variance"):
        assert fit[name]["n_increments"] == 10 and fit[name]["status"] == 0 and fit[name]["D_ml"] > 0, name
    assert fit["long"]["n_increments"] == lc.LONG_ROWS - 1 and fit["long"]["status"] == 0


def test_a_dropped_row_is_a_gap(edge_batch):
    """the fit of a range with unusable rows is the fit of the range without those rows, bit for bit"""
    b, fit = edge_batch
    k = b["names"].index("gaps and unusable rows")
    a, e = b["offsets"][k], b["offsets"][k + 1]
    u = b["use"][a:e]
    assert 0 < u.sum() < len(u)
    alone = M.estimate_diffusion_ml(b["pos"][a:e][u], np.array([0, u.sum()]), b["var"][a:e][u], frames=b["frames"][a:e][u],
                                    dt=lc.BATCH_DT, blur=lc.BATCH_R)
    for key, v in alone.items():
        assert v[0] == fit["gaps and unusable rows"][key], key


def test_a_track_that_does_not_move(edge_batch):
    b, fit = edge_batch
    for name in ("identical positions", "identical positions, no variance", "immobile within its noise"):
        got = fit[name]
        assert got["status"] == 2 and got["D_ml"] == 0.0 and np.isnan(got["D_ml_std"]), name
    assert np.isfinite(fit["identical positions"]["loglik"])
    assert fit["identical positions, no variance"]["loglik"] == -np.inf   # a point mass: every candidate is rejected


def test_omitted_arguments_are_their_defaults(edge_batch):
    b, _ = edge_batch
    pos, off, n = b["pos"], b["offsets"], len(b["pos"])
    pos = np.where(np.isfinite(pos), pos, 1.0)
    kw = dict(dt=lc.BATCH_DT, blur=lc.BATCH_R)
    consecutive = np.concatenate([np.arange(e - a) for a, e in zip(off[:-1], off[1:])])
    pairs = [(M.estimate_diffusion_ml(pos, off, **kw),
              M.estimate_diffusion_ml(pos, off, np.zeros((n, 2)), frames=consecutive, use=np.ones(n, bool), **kw)),
             (M.estimate_diffusion_ml(pos, off, 0.01, **kw), M.estimate_diffusion_ml(pos, off, np.full((n, 2), 0.01), **kw)),
             (M.estimate_diffusion_ml(pos, off, np.full(n, 0.01), **kw), M.estimate_diffusion_ml(pos, off, np.full((n, 2), 0.01), **kw))]
    for got, want in pairs:
        for key in want:
            assert np.array_equal(got[key], want[key], equal_nan=True), key
    t = M.estimate_diffusion_ml(torch.from_numpy(pos), torch.from_numpy(off), 0.01, **kw)
    assert all(torch.is_tensor(v) for v in t.values())
    assert np.array_equal(t["D_ml"].numpy(), pairs[1][0]["D_ml"], equal_nan=True)
    assert t["status"].dtype == t["n_increments"].dtype == torch.int64
    empty = M.estimate_diffusion_ml(np.zeros((0, 2)), np.zeros(1, np.int64))
    assert all(len(v) == 0 for v in empty.values())


# ----------------------------------------------------------------------------------------------------------------------
# arguments
# ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    pos, off = np.zeros((6, 2)), np.array([0, 6])
    for kw, match in (({"blur": 0.3}, "blur"), ({"blur": -0.1}, "blur"), ({"dt": 0.0}, "dt"), ({"dt": float("inf")}, "dt"),
                      ({"variances": np.zeros((5, 2))}, "variances"), ({"variances": np.zeros((6, 3))}, "variances"),
                      ({"variances": -1.0}, "variance"), ({"frames": np.arange(5)}, "frames"),
                      ({"frames": np.arange(6.0)}, "integers"), ({"frames": np.array([0, 1, 2, 2, 4, 5])}, "rise"),
                      ({"use": np.ones(5, bool)}, "use"), ({"use": np.ones(6, np.int32)}, "use"),
                      ({"frames": torch.arange(6)}, "all be tensors or all be arrays")):
        with pytest.raises(ValueError, match=match):
            M.estimate_diffusion_ml(pos, off, **kw)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        M.estimate_diffusion_ml(np.zeros((6, 3)), off)
    with pytest.raises(ValueError, match="offsets"):
        M.estimate_diffusion_ml(pos, np.array([0, 5]))
    with pytest.raises(ValueError, match="offsets"):
        M.estimate_diffusion_ml(pos, np.array([0, 4, 3, 6]))
    # frames may fall back between two ranges
    M.estimate_diffusion_ml(pos, np.array([0, 3, 6]), frames=np.array([5, 6, 9, 0, 1, 2]))
    # estimate_track_diffusion(ml=...): checked before the movie is
    movie = torch.zeros(4, 32, 32)
    for ml in (0.1, {"R": 0.1}, {"blur": 0.3}, {"sigma2": "bound"}, {"sigma2": -1.0}):
        with pytest.raises(ValueError, match="ml"):
            T.estimate_track_diffusion(movie, None, 4, ml=ml)
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(movie, None, 4, ml={"sigma2": "crlb"})
    with pytest.raises(ValueError, match="CUDA movie"):
        T.estimate_track_diffusion(movie, None, 4, ml={})


# ----------------------------------------------------------------------------------------------------------------------
# the pieces that the maximum-likelihood fits share (helpers/msd._ml_usable, _ml_hessian; csrc/track_ml.h for the kernels)
# ----------------------------------------------------------------------------------------------------------------------
def test_the_usable_row_rule_row_by_row():
    """_ml_usable against the rule stated one row at a time: 40 rows that hold every way a row can be unusable, three ranges
    of which one is empty, and var, frames and use each left out in turn"""
    N = 40
    pos = np.stack([10.0 + 0.25 * np.arange(N), 50.0 - 0.5 * np.arange(N)], axis=1)
    var, use, frames = np.full((N, 2), 0.01), np.ones(N, bool), 3 * np.arange(N)
    use[[1, 23]] = False
    pos[3, 0], pos[4, 1], pos[23, 0] = np.nan, np.nan, np.nan
    pos[6, 0], pos[7, 1], pos[8, 0], pos[9, 1] = np.inf, -np.inf, -np.inf, np.inf
    var[11, 0], var[12, 1], var[25, 0] = -1e-3, -1e-300, -np.inf
    var[14, 0], var[15, 1] = np.nan, np.nan
    var[17, 0], var[18, 1] = np.inf, np.inf
    var[20, 0], var[21, 1] = -0.0, -0.0                                     # usable: -0.0 >= 0
    var[30], var[31, 1] = 0.0, 1e300                                       # usable
    offsets = np.array([0, 16, 16, N])
    by_flag, by_pos, by_var = {1, 23}, {3, 4, 6, 7, 8, 9, 23}, {11, 12, 14, 15, 17, 18, 25}

    def rule(r, var, use):
        if use is not None and not use[r]:
            return False
        if not (abs(float(pos[r, 0])) < float("inf") and abs(float(pos[r, 1])) < float("inf")):
            return False
        return var is None or all(0.0 <= float(v) < float("inf") for v in var[r])

    for v, f, u, out in ((var, frames, use, by_flag | by_pos | by_var), (None, frames, use, by_flag | by_pos),
                         (var, None, use, by_flag | by_pos | by_var), (var, frames, None, by_pos | by_var)):
        got = M._ml_usable(pos, v, f, u, offsets)
        assert len(got) == 3 and len(got[1]) == 0
        for k, rows in enumerate(got):
            assert rows.dtype.kind == "i"
            want = [r for r in range(int(offsets[k]), int(offsets[k + 1])) if rule(r, v, u)]
            assert rows.tolist() == want, (k, rows.tolist(), want)
        assert sorted(set(range(N)) - set(np.concatenate(got).tolist())) == sorted(out)       # the rule itself is the one meant


def test_the_hessian_of_an_exact_quadratic():
    """_ml_hessian on a u^2 + b v^2 + c u v + d sampled at the stencil's points with h = 1 / 64: with dyadic a, b, c every
    difference is exact, so the entries are a, b and c / 2 to the bit"""
    h = 1.0 / 64.0
    quads = [(1.5, 0.75, -0.5, 1000.0), (0.25, 3.0, 1.0, -7.0), (-0.5, 2.0, 0.25, 0.0), (1.0, 1.0, 2.0, 3.0)]
    c = np.array([[a * u * u + b * v * v + m * u * v + d for u in (-h, 0.0, h) for v in (-h, 0.0, h)] for a, b, m, d in quads])
    uu, vv, uv, det, pd = M._ml_hessian(c)
    for i, (a, b, m, d) in enumerate(quads):
        want = np.array([a, b, 0.5 * m, a * b - (0.5 * m) * (0.5 * m)])
        assert np.array([uu[i], vv[i], uv[i], det[i]]).tobytes() == want.tobytes(), (i, uu[i], vv[i], uv[i], det[i])
        one = M._ml_hessian(c[i])                                          # one range: the fit of the anomalous exponent
        assert np.array(one[:4]).tobytes() == want.tobytes() and bool(one[4]) == bool(pd[i])
    assert pd.tolist() == [True, True, False, False]                       # a < 0; det = 0
