"""CPU: the host restatement of the Poisson maximum-likelihood fit (helpers/tracking._fit_mle_numpy) against the scalar oracle
of tests/localize_common.py, its efficiency against the Cramer-Rao bound, the camera model of simulate_movie, and the
arguments of everything the localisation precision is threaded through."""
import math

import numpy as np
import pytest
import torch

import localize_common as LC
from moleculardiffusion_mivit_amd.helpers import generation as G
from moleculardiffusion_mivit_amd.helpers import tracking as T


def _with_dark_pixels(name, n):
    """n patches of a case with a few pixels at 0 ADU: below the offset where there is one, d = 0 (+ read_var) either way."""
    patches = LC.case_patches(name, n).copy()
    P = patches.shape[1]
    patches[:, 0, 0] = 0.0
    patches[:, P - 1, 1] = 0.0
    patches[:, P // 2, P // 2 - 1] = 0.0
    return patches


def _random_parameters(name, n, seed):
    P, photons, bg, sigma, _, _, _, _, _ = LC.CASES[name]
    rng = np.random.default_rng(seed)
    return np.stack([photons * rng.uniform(0.5, 1.5, n), P // 2 + rng.uniform(-1.0, 1.0, n), P // 2 + rng.uniform(-1.0, 1.0, n),
                     sigma * rng.uniform(0.8, 1.3, n), bg * rng.uniform(0.5, 1.5, n)], axis=1)


def test_the_oracle_gradient_is_the_derivative_of_its_deviance():
    """central differences of the oracle's own deviance: guards the oracle's analytic derivatives, on which all else rests"""
    name = "p9_camera"
    kw = LC.camera_kwargs(name)
    patch = LC.case_patches(name, 1)[0]
    p = _random_parameters(name, 1, 0)[0]
    _, grad, _, _, _ = LC.oracle(patch, p, kw["gain"], kw["offset"], kw["read_var"], True)
    for k in range(5):
        h = 1e-5 * max(abs(p[k]), 1.0)
        hi, lo = p.copy(), p.copy()
        hi[k] += h
        lo[k] -= h
        num = (LC.oracle(patch, hi, kw["gain"], kw["offset"], kw["read_var"])[0]
               - LC.oracle(patch, lo, kw["gain"], kw["offset"], kw["read_var"])[0]) / (2 * h)
        # the deviance is twice the negative log likelihood, the gradient is that of the log likelihood's negative
        assert abs(num - 2.0 * grad[k]) <= 1e-6 * max(abs(2.0 * grad[k]), 1.0), (k, num, 2.0 * grad[k])


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_cost_gradient_and_matrix_equal_the_oracle(name):
    kw = LC.camera_kwargs(name)
    n = 4
    patches = _with_dark_pixels(name, n)
    if kw["offset"] > 0:
        assert (patches < kw["offset"]).any()
    p = _random_parameters(name, n, 1)
    if not kw["fit_sigma"]:
        p[:, 3] = kw["sigma0"]
    d = T._mle_data(patches, kw["gain"], kw["offset"], kw["read_var"])
    assert (d == kw["read_var"]).any()
    cost, g, A, bad, _ = T._mle_normal(d, p, kw["read_var"], kw["fit_sigma"])
    assert not bad.any()
    free = [0, 1, 2, 3, 4] if kw["fit_sigma"] else [0, 1, 2, 4]
    for i in range(n):
        dev, grad, fisher, dev_abs, grad_abs = LC.oracle(patches[i], p[i], kw["gain"], kw["offset"], kw["read_var"],
                                                         kw["fit_sigma"])
        assert abs(cost[i] - dev) <= LC.ROUNDING_RTOL * dev_abs
        full = A[i] + np.tril(A[i], -1).T
        for a, fa in enumerate(free):
            assert abs(g[i, fa] - grad[a]) <= LC.ROUNDING_RTOL * grad_abs[a]
            for c, fc in enumerate(free):
                assert abs(full[fa, fc] - fisher[a, c]) <= LC.ROUNDING_RTOL * math.sqrt(fisher[a, a] * fisher[c, c])
        if not kw["fit_sigma"]:
            assert g[i, 3] == 0.0 and full[3, 3] == 1.0 and not full[3, [0, 1, 2, 4]].any()


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_returned_optimum_and_crlb_against_the_oracle(name):
    kw = LC.camera_kwargs(name)
    n = LC.TABLE_N                                           # every returned optimum of the table
    params, crlb, deviance, status, iterations = LC.case_reference(name)
    assert len(status) == n and (status == 0).all()
    assert iterations.max() < T.FIT_MAX_ITER
    free = [0, 1, 2, 3, 4] if kw["fit_sigma"] else [0, 1, 2, 4]
    for i in range(n):
        dev, grad, fisher, dev_abs, _ = LC.oracle(LC.case_patches(name)[i], params[i], kw["gain"], kw["offset"], kw["read_var"],
                                                  kw["fit_sigma"])
        step = np.linalg.solve(fisher, -grad)
        assert (np.abs(step) <= 2.0 * T.FIT_XTOL * LC.step_scale(params[i])[free]).all(), (i, step)
        assert abs(deviance[i] - dev) <= LC.ROUNDING_RTOL * dev_abs
        np.testing.assert_allclose(crlb[i][free], np.diag(np.linalg.inv(fisher)), rtol=LC.CRLB_RTOL, atol=0.0)
        if not kw["fit_sigma"]:
            assert crlb[i, 3] == 0.0 and params[i, 3] == kw["sigma0"]


# measured with the restatement (x, y): bright_free_sigma 1.0206, 1.0061; dim_fixed_sigma 0.9892, 1.0002
@pytest.mark.parametrize("name", sorted(LC.EFFICIENCY))
def test_the_fit_reaches_the_cramer_rao_bound(name):
    LC.check_efficiency(name, *LC.efficiency_figures(name, T._fit_mle_numpy))


def test_dispatch_keeps_the_kind_of_the_input():
    name = "p7"
    kw = LC.camera_kwargs(name)
    ref = LC.case_reference(name)
    out = T.fit_spots_mle(torch.from_numpy(LC.case_patches(name, 8).copy()), **kw)
    assert all(torch.is_tensor(o) for o in out)
    assert [o.dtype for o in out] == [torch.float64, torch.float64, torch.float64, torch.int32, torch.int32]
    for o, r in zip(out, ref):
        np.testing.assert_array_equal(o.numpy(), r[:8])
    out = T.fit_spots_mle(LC.case_patches(name, 0), **kw)
    assert [o.shape for o in out] == [(0, 5), (0, 5), (0,), (0,), (0,)]


def test_degenerate_patches_end_with_a_status():
    P = 7
    patches = np.stack([np.zeros((P, P)), np.full((P, P), 40.0), np.full((P, P), 90.0), LC.case_patches("p7", 1)[0],
                        np.full((P, P), np.nan)]).astype(np.float32)
    patches[3, 2, 2] = np.inf
    for offset in (0.0, 100.0):
        params, crlb, deviance, status, iterations = T._fit_mle_numpy(patches, offset=offset)
        assert status[3] == 3 and status[4] == 3
        assert np.isfinite(params[:3]).all() and set(status[:3]) <= {0, 1, 2}
        assert np.isnan(crlb[status != 0]).all()
        assert (iterations <= T.FIT_MAX_ITER).all()
    assert status[0] == status[1] == status[2] == 1          # below the offset: no photon to start from


def test_argument_errors_of_the_fit():
    ok = np.ones((2, 7, 7), np.float32)
    for bad in ({"gain": 0.0}, {"gain": -1.0}, {"gain": float("inf")}, {"offset": float("nan")}, {"offset": float("inf")},
                {"read_var": -1.0}, {"read_var": float("nan")}, {"sigma0": 0.2}, {"sigma0": 7.0}, {"xtol": 0.0}, {"xtol": 1e-3}):
        with pytest.raises(ValueError):
            T.fit_spots_mle(ok, **bad)
    with pytest.raises(ValueError):
        T.fit_spots_mle(np.ones((2, 8, 8), np.float32))
    with pytest.raises(ValueError):
        T.fit_spots_mle(np.ones((2, 17, 17), np.float32))
    with pytest.raises(ValueError):
        T.fit_spots_mle(np.ones((2, 7, 9), np.float32))
    ys = xs = np.zeros(2)
    with pytest.raises(ValueError):
        T.refine_localizations(ok, ys, xs, method="ml")
    with pytest.raises(ValueError):
        T.refine_localizations(ok, ys, xs, method="mle", camera={"background": 1.0})
    with pytest.raises(ValueError):
        T.refine_localizations(ok, ys, xs, method="mle", camera=[1.0])
    with pytest.raises(ValueError):
        T.refine_localizations(ok, ys, xs, camera={"gain": 2.0})
    with pytest.raises(ValueError):
        T.refine_localizations_tensors(torch.ones(2, 7, 7), ys, xs, method="mle")      # needs CUDA patches


def test_argument_errors_of_estimate_track_diffusion():
    """checked before the movie is: a CPU movie would be refused next"""
    movie = torch.zeros(4, 32, 32)
    with pytest.raises(ValueError, match="localization"):
        T.estimate_track_diffusion(movie, None, 4, localization={"background": 1.0})
    with pytest.raises(ValueError, match="localization"):
        T.estimate_track_diffusion(movie, None, 4, localization=3.0)
    with pytest.raises(ValueError, match="refine"):
        T.estimate_track_diffusion(movie, None, 4, localization={}, refine=False)
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(movie, None, 4, states={"K": 2, "sigma2": "crlb"})
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(movie, None, 4, states={"K": 2, "sigma2": "bound"}, localization={})


def test_refine_localizations_default_is_the_least_squares_path():
    import tracking_common as TC
    patches = TC.spot_patches(40, 9)
    ys, xs = np.arange(40) + 20, np.arange(40) + 30
    params, peak, status = T.refine_gaussian_patches(patches)
    half = 4
    okf = status == 0
    want = {"x_refined": np.where(okf, xs - half + params[:, 1], xs.astype(np.float64)),
            "y_refined": np.where(okf, ys - half + params[:, 2], ys.astype(np.float64)),
            "psf_size": np.where(okf, params[:, 3], float(T.FALLBACK_PSF_SIZE)), "max_intensity": peak, "status": status}
    for got in (T.refine_localizations(patches, ys, xs), T.refine_localizations(patches, ys, xs, method="lsq")):
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def test_refine_localizations_mle_columns_and_fallback():
    name = "p9_camera"
    kw = LC.camera_kwargs(name)
    patches = LC.case_patches(name, 6).copy()
    patches[2] = np.nan
    ys, xs = np.arange(6) + 20, np.arange(6) + 30
    res = T.refine_localizations(patches, ys, xs, method="mle", camera=kw)
    params, crlb, deviance, status, _ = T._fit_mle_numpy(patches, **kw)
    assert status[2] == 3 and (np.delete(status, 2) == 0).all()
    assert set(res) == {"x_refined", "y_refined", "psf_size", "max_intensity", "status", "x_std", "y_std", "photons",
                        "background", "deviance"}
    good = status == 0
    np.testing.assert_array_equal(res["x_refined"][good], (xs - 4 + params[:, 1])[good])
    np.testing.assert_array_equal(res["y_refined"][good], (ys - 4 + params[:, 2])[good])
    np.testing.assert_array_equal(res["x_std"][good], np.sqrt(crlb[good, 1]))
    np.testing.assert_array_equal(res["y_std"][good], np.sqrt(crlb[good, 2]))
    np.testing.assert_array_equal(res["photons"][good], params[good, 0])
    np.testing.assert_array_equal(res["background"][good], params[good, 4])
    np.testing.assert_array_equal(res["deviance"][good], deviance[good])
    assert res["x_refined"][2] == xs[2] and res["y_refined"][2] == ys[2] and res["psf_size"][2] == T.FALLBACK_PSF_SIZE
    for k in ("x_std", "y_std", "photons", "background", "deviance"):
        assert np.isnan(res[k][2]), k


# ----------------------------------------------------------------------------------------------------------------------
# the camera model of simulate_movie
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", [{"background": 12.0}, {"background": 7.0, "gain": 2.5, "offset": 90.0, "read_noise": 3.0}])
def test_an_empty_field_has_the_camera_statistics(camera):
    movie, truth = G.simulate_movie(0, 8, 64, 64, 0.1, 2, camera=camera, generator=torch.Generator().manual_seed(4))
    cam = truth["camera"]
    assert cam == {"background": camera["background"], "gain": camera.get("gain", 1.0), "offset": camera.get("offset", 0.0),
                   "read_noise": camera.get("read_noise", 0.0)}
    x = movie.double().numpy().ravel()
    n, g, b, r = x.size, cam["gain"], cam["background"], cam["read_noise"]
    var = g * g * b + r * r
    kappa4 = g ** 4 * b                                           # fourth cumulant: Poisson's is its mean, the Gaussian's 0
    assert abs(x.mean() - (cam["offset"] + g * b)) <= 4.0 * math.sqrt(var / n)
    assert abs(x.var() - var) <= 4.0 * math.sqrt((kappa4 + 2.0 * var * var) / n)
    assert truth["photons"].shape == (0,)


def test_camera_none_is_the_call_without_it():
    args = (3, 5, 48, 48, 0.05, 3)
    a, ta = G.simulate_movie(*args, generator=torch.Generator().manual_seed(9))
    b, tb = G.simulate_movie(*args, generator=torch.Generator().manual_seed(9), camera=None)
    assert a.numpy().tobytes() == b.numpy().tobytes()
    assert sorted(ta) == sorted(tb) and "camera" not in tb and "photons" not in tb
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k


def test_camera_truth_photons_and_draw_order():
    args = (3, 5, 48, 48, 0.05, 3)
    props = {"particle_intensity": [300.0, 5.0]}
    m0, t0 = G.simulate_movie(*args, image_props=props, generator=torch.Generator().manual_seed(9))
    m1, t1 = G.simulate_movie(*args, image_props=props, generator=torch.Generator().manual_seed(9),
                              camera={"background": 10.0, "gain": 2.0, "offset": 100.0})
    assert torch.equal(t0["pos"], t1["pos"]) and torch.equal(t0["amp"], t1["amp"])      # drawn after the amplitudes
    full = dict(G.DEFAULT_IMAGE_PROPS)
    sigma = G.psf_sigma_hr(full) / full["upsampling_factor"]
    want = t1["amp"].double().sum(-1)[t1["particle_id"], t1["frame"]] * 2.0 * math.pi * sigma ** 2
    assert torch.allclose(t1["photons"], want, rtol=1e-14, atol=0.0)
    assert abs(float(t1["photons"].mean()) / (300.0 * 2.0 * math.pi * sigma ** 2) - 1.0) < 0.02
    counts = (m1.double() - 100.0) / 2.0
    assert torch.equal(counts, counts.round()) and float(counts.min()) >= 0.0            # gain * integer photons + offset


def test_argument_errors_of_the_camera():
    args = (1, 2, 40, 40, 0.05, 2)
    for bad in ({"gain": 2.0}, {"background": -1.0}, {"background": 1.0, "gain": 0.0}, {"background": 1.0, "read_noise": -1.0},
                {"background": 1.0, "offset": float("nan")}, {"background": 1.0, "read_var": 1.0}, {"background": "many"}, 10.0):
        with pytest.raises(ValueError):
            G.simulate_movie(*args, camera=bad)


# ----------------------------------------------------------------------------------------------------------------------
# two particles on a camera movie: the reported error bar against the truth table
# ----------------------------------------------------------------------------------------------------------------------
# measured on the CPU with torch's draws at MOVIE_SEED = 1: 0.9900 (y), 1.0316 (x) on 200 rows, band [0.85, 1.15]
def test_error_bars_on_a_two_particle_camera_movie():
    patches, iy, ix, y, x, sigma = LC.movie_patches_and_truth()
    res = T.refine_localizations(patches, iy, ix, method="mle", camera=LC.movie_fit_camera(sigma))
    assert len(y) == 200 and (res["status"] == 0).all()
    ry = math.sqrt(np.mean(((res["y_refined"] - y) / res["y_std"]) ** 2))
    rx = math.sqrt(np.mean(((res["x_refined"] - x) / res["x_std"]) ** 2))
    print(f"two-particle movie: RMS of error / std y {ry:.4f} x {rx:.4f}; photons fitted / truth "
          f"{np.mean(res['photons']) / float(LC.two_particle_movie()[1]['photons'].mean()):.4f}")
    assert LC.MOVIE_BAND[0] <= ry <= LC.MOVIE_BAND[1] and LC.MOVIE_BAND[0] <= rx <= LC.MOVIE_BAND[1]
