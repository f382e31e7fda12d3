"""GPU: the Poisson maximum-likelihood fit kernel (csrc/localize.hip, ops.fit_spots_mle) against the host restatement
(helpers/tracking._fit_mle_numpy) on the case table of tests/localize_common.py -- status and iterations equal, parameters, CRLB
and deviance at KERNEL_FIT_RTOL --, its behaviour (the same bits alone, in a batch and twice; NaN and empty patches), its
arguments at the wrapper and at the C entry, its efficiency, and the localisation precision carried through
refine_localizations_tensors and estimate_track_diffusion."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import localize_common as LC
import track_diffusion_common as dc
import tracking_common as tc
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as G
from moleculardiffusion_mivit_amd.helpers import models as M
from moleculardiffusion_mivit_amd.helpers import msd as MSD
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

COLUMNS = ("photons", "x0", "y0", "sigma", "background")
# every batch size at which the launch takes another shape: 1 .. 257 run one lane per wave, 600 two, 5000 sixteen, and
# 64 * 256 + 116 fills the waves
SIZES = (0, 1, 63, 64, 65, 257, 600, 5000, 64 * 256 + 116)


def _kernel(patches, **kw):
    out = ops.fit_spots_mle(torch.tensor(patches).cuda(), **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _worst(got, want):
    """worst relative difference per column, where both are finite; NaN positions must agree"""
    if len(got) == 0:
        return np.zeros(1)
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want == got, 0.0, np.abs(got - want) / np.abs(want))
    return np.nanmax(rel, axis=0)


# the batches above the table repeat it, so one case per mode covers those launch shapes
BATCHES = [(name, n) for name in sorted(LC.CASES) for n in SIZES if n <= LC.TABLE_N or name in ("p7", "p9_fixed_camera")]


@pytest.mark.parametrize("name,n", BATCHES)
def test_kernel_against_the_restatement(name, n):
    kw = LC.camera_kwargs(name)
    params, crlb, deviance, status, iterations = _kernel(LC.case_patches(name, n), **kw)
    want = [LC.tiled(a, n) if n else a[:0] for a in LC.case_reference(name)]
    assert params.shape == (n, 5) and crlb.shape == (n, 5) and deviance.shape == status.shape == iterations.shape == (n,)
    assert status.dtype == iterations.dtype == np.int32
    assert np.array_equal(status, want[3]) and np.array_equal(iterations, want[4])
    wp, wc, wd = _worst(params, want[0]), _worst(crlb, want[1]), _worst(deviance, want[2])
    print(f"{name} n = {n}: worst relative difference, parameters", dict(zip(COLUMNS, wp)), "CRLB", dict(zip(COLUMNS, wc)),
          "deviance", float(wd[0]))
    assert (wp <= tc.KERNEL_FIT_RTOL).all() and (wc <= tc.KERNEL_FIT_RTOL).all() and (wd <= tc.KERNEL_FIT_RTOL).all()
    if n and not kw["fit_sigma"]:
        assert (params[:, 3] == kw["sigma0"]).all() and (crlb[:, 3] == 0.0).all()


@pytest.mark.parametrize("name", ["p7", "p15_camera"])
def test_same_bits_alone_in_a_batch_and_twice(name):
    kw = LC.camera_kwargs(name)
    patches = LC.case_patches(name, 64 * 256 + 116 if name == "p7" else LC.TABLE_N)
    first, second = _kernel(patches, **kw), _kernel(patches, **kw)
    for a, b in zip(first, second):
        assert dc.same_bits(a.astype(np.float64), b.astype(np.float64))
    for k in (0, 100, LC.TABLE_N - 1):
        alone = _kernel(patches[k:k + 1], **kw)
        for a, b in zip(first, alone):
            assert dc.same_bits(a[k:k + 1].astype(np.float64), b.astype(np.float64)), k
    if len(patches) > LC.TABLE_N:                           # the same patch in another wave and lane
        for a in first:
            assert dc.same_bits(a[:LC.TABLE_N].astype(np.float64), a[LC.TABLE_N:2 * LC.TABLE_N].astype(np.float64))


def _unfactorable(P, sigma):
    """([2, P, P] patches, gain): two noiseless spots whose brightest pixel is 1.5e300 photons through a gain of 1e-291.  The
    deviance of the start stays below 1e300 (2e299 at P = 3, where it is largest), the position entries of the Fisher matrix
    (about N^2 / mu) do not, so no damping makes it factor: 14 failed factorisations, each counted as an iteration, take lambda
    past 1e10.  Both margins are factors of about 5, far from anything rounding decides."""
    img = LC.expected_image(P, 1000.0, 10.0, sigma, P // 2 + np.array([0.05, -0.04]), P // 2 + np.array([-0.03, 0.02]))
    return (img * (1.5e9 / img.max(axis=(1, 2), keepdims=True))).astype(np.float32), 1e-291


@pytest.mark.parametrize("name", ["p3_fixed", "p15_camera"])
def test_the_iteration_cap_and_a_matrix_that_never_factors(name):
    """The two exits of the damped loop that no patch of the table takes: with xtol = 1e-300 no step is ever small, so the
    fit runs to the iteration cap at its optimum (status 2, 100 iterations); a matrix past 1e300 ends as status 1 after 14."""
    kw = LC.camera_kwargs(name)
    P = LC.CASES[name][0]
    patches, gain = _unfactorable(P, kw["sigma0"])
    for pat, k, status, iters in ((LC.case_patches(name, 5), dict(kw, xtol=1e-300), 2, 100),
                                  (patches, dict(kw, gain=gain, offset=0.0, read_var=0.0), 1, 14)):
        want = T._fit_mle_numpy(pat, **k)
        assert (want[3] == status).all() and (want[4] == iters).all()
        params, crlb, deviance, st, it = _kernel(pat, **k)
        assert np.array_equal(st, want[3]) and np.array_equal(it, want[4])
        wp, wd = _worst(params, want[0]), _worst(deviance, want[2])
        print(f"{name} status {status}: worst relative difference, parameters", dict(zip(COLUMNS, wp)), "deviance", float(wd[0]))
        assert (wp <= tc.KERNEL_FIT_RTOL).all() and (wd <= tc.KERNEL_FIT_RTOL).all()
        assert np.isnan(crlb).all() and np.isnan(want[1]).all()


def test_a_nan_patch_has_status_3_and_leaves_its_neighbours_alone():
    name = "p9_camera"
    kw = LC.camera_kwargs(name)
    patches = LC.case_patches(name, 130).copy()
    clean = _kernel(patches, **kw)
    for k in (0, 64, 129):
        patches[k, 3, 5] = np.nan
    patches[65] = np.inf
    got = _kernel(patches, **kw)
    bad = np.zeros(130, bool)
    bad[[0, 64, 65, 129]] = True
    assert (got[3][bad] == 3).all() and (got[4][bad] == 0).all()
    assert np.isnan(got[0][bad]).all() and np.isnan(got[1][bad]).all() and np.isnan(got[2][bad]).all()
    for a, b in zip(got, clean):
        assert dc.same_bits(a[~bad].astype(np.float64), b[~bad].astype(np.float64))


def test_patches_without_a_spot_end_with_a_status():
    P = 7
    patches = np.stack([np.zeros((P, P)), np.full((P, P), 40.0), np.full((P, P), 90.0)]).astype(np.float32)
    for offset in (0.0, 100.0):
        got = _kernel(patches, offset=offset)
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all() and set(got[3]) <= {0, 1, 2}
        assert (got[4] <= T.FIT_MAX_ITER).all() and np.isnan(got[1][got[3] != 0]).all()
    assert (got[3] == 1).all() and (got[4] == 0).all()       # below the offset: no photon to start from, no iteration


def test_arguments_are_checked_by_the_wrapper_and_by_the_c_entry():
    ok = torch.ones(2, 7, 7, device="cuda")
    for bad in ({"gain": 0.0}, {"gain": -1.0}, {"gain": float("inf")}, {"gain": float("nan")}, {"offset": float("nan")},
                {"offset": float("inf")}, {"read_var": -1.0}, {"read_var": float("nan")}, {"sigma0": 0.2}, {"sigma0": 7.0},
                {"sigma0": float("nan")}, {"xtol": 0.0}, {"xtol": 1e-3}):
        with pytest.raises(ValueError):
            ops.fit_spots_mle(ok, **bad)
        with pytest.raises(ValueError):
            T.fit_spots_mle(ok, **bad)
    with pytest.raises(N.MivitError, match="patch side"):
        ops.fit_spots_mle(torch.ones(2, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        T.fit_spots_mle(torch.ones(2, 8, 8, device="cuda"))
    with pytest.raises(N.MivitError, match="patch side"):
        ops.fit_spots_mle(torch.ones(2, 17, 17, device="cuda"), sigma0=1.0)
    with pytest.raises(ValueError):
        ops.fit_spots_mle(torch.ones(2, 7, 9, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        ops.fit_spots_mle(ok.double())
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ops.fit_spots_mle(ok.cpu())
    # the C entry refuses the same before any launch: the outputs keep their sentinel
    outs = [torch.full((2, 5), -7.0, dtype=torch.float64, device="cuda"), torch.full((2, 5), -7.0, dtype=torch.float64, device="cuda"),
            torch.full((2,), -7.0, dtype=torch.float64, device="cuda"), torch.full((2,), -7, dtype=torch.int32, device="cuda"),
            torch.full((2,), -7, dtype=torch.int32, device="cuda")]
    ptr = [o.data_ptr() for o in outs]

    def entry(n=2, P=7, gain=1.0, offset=0.0, read_var=0.0, sigma0=1.0, fit_sigma=1, xtol=1e-11, patches=ok.data_ptr(), out0=ptr[0]):
        return N.lib.mivit_fit_spots_mle(patches, n, P, gain, offset, read_var, sigma0, fit_sigma, xtol, out0, *ptr[1:], None)

    for bad in ({"n": -1}, {"P": 8}, {"P": 1}, {"P": 17}, {"gain": 0.0}, {"gain": float("nan")}, {"gain": float("inf")},
                {"offset": float("nan")}, {"offset": float("-inf")}, {"read_var": -1e-9}, {"read_var": float("nan")},
                {"sigma0": 0.2}, {"sigma0": 7.0}, {"sigma0": float("nan")}, {"fit_sigma": 2}, {"xtol": 0.0}, {"xtol": 1e-7},
                {"xtol": float("nan")}, {"patches": None}, {"out0": None}):
        assert entry(**bad) != 0, bad
        assert N.last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -7).all())
    assert entry(n=0, patches=None, out0=None) == 0
    assert entry() == 0
    torch.cuda.synchronize()
    assert bool((outs[3] >= 0).all())


@pytest.mark.parametrize("name", sorted(LC.EFFICIENCY))
def test_the_kernel_reaches_the_cramer_rao_bound(name):
    LC.check_efficiency(name, *LC.efficiency_figures(name, _kernel))


def test_error_bars_on_a_two_particle_camera_movie():
    """the movie is drawn on the CPU (torch's draws there, MOVIE_SEED) and moved: measured 0.9900 (y), 1.0316 (x) as on the CPU"""
    patches, iy, ix, y, x, sigma = LC.movie_patches_and_truth()
    camera = LC.movie_fit_camera(sigma)
    want = T.refine_localizations(patches, iy, ix, method="mle", camera=camera)
    got = T.refine_localizations_tensors(torch.from_numpy(patches).cuda(), torch.from_numpy(iy).cuda(), torch.from_numpy(ix).cuda(),
                                         method="mle", camera=camera)
    assert set(got) == set(want) and all(v.is_cuda for v in got.values())
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert (got["status"] == 0).all() and np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["max_intensity"], want["max_intensity"])
    for k in ("x_refined", "y_refined", "psf_size", "x_std", "y_std", "photons", "background", "deviance"):
        assert got[k].dtype == np.float64
        assert np.allclose(got[k], want[k], rtol=tc.KERNEL_FIT_RTOL, atol=0.0), k
    ry = float(np.sqrt(np.mean(((got["y_refined"] - y) / got["y_std"]) ** 2)))
    rx = float(np.sqrt(np.mean(((got["x_refined"] - x) / got["x_std"]) ** 2)))
    print(f"two-particle movie on the kernel: RMS of error / std y {ry:.4f} x {rx:.4f}")
    assert LC.MOVIE_BAND[0] <= ry <= LC.MOVIE_BAND[1] and LC.MOVIE_BAND[0] <= rx <= LC.MOVIE_BAND[1]
    # the fallback, and the default path untouched by the new arguments
    broken = torch.from_numpy(patches[:3].copy()).cuda()
    broken[1] = float("nan")
    res = T.refine_localizations_tensors(broken, torch.from_numpy(iy[:3]).cuda(), torch.from_numpy(ix[:3]).cuda(), method="mle",
                                         camera=camera)
    assert res["status"].tolist() == [0, 3, 0] and float(res["x_refined"][1]) == ix[1] and float(res["psf_size"][1]) == T.FALLBACK_PSF_SIZE
    assert all(bool(torch.isnan(res[k][1])) for k in ("x_std", "y_std", "photons", "background", "deviance"))
    a = T.refine_localizations_tensors(broken, torch.from_numpy(iy[:3]).cuda(), torch.from_numpy(ix[:3]).cuda())
    b = T.refine_localizations_tensors(broken, torch.from_numpy(iy[:3]).cuda(), torch.from_numpy(ix[:3]).cuda(), method="lsq")
    assert set(a) == set(b) == {"x_refined", "y_refined", "psf_size", "max_intensity", "status"}
    for k in a:
        assert dc.same_bits(a[k].double().cpu().numpy(), b[k].double().cpu().numpy()), k


# ----------------------------------------------------------------------------------------------------------------------
# estimate_track_diffusion(localization=)
# ----------------------------------------------------------------------------------------------------------------------
SEQ_LEN, PATCH, BATCH, DT = 5, 9, 16, 0.03
CAMERA = {"background": 10.0, "gain": 2.0, "offset": 100.0, "read_noise": 2.0}


def _model():
    torch.manual_seed(0)
    return M.GeneralTransformer(M.LinearProjectionEmbedding, dict(patch_size=PATCH, embed_dim=64), 64, 4, 128, 1,
                                partial(M.MLPHead, hidden_dim=128, output_dim=1), F.relu, precision="fp32").cuda()


def _bits(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and dc.same_bits(a.double().cpu().numpy(), b.double().cpu().numpy())
    if isinstance(a, np.ndarray):
        return dc.same_bits(a.astype(np.float64), np.asarray(b).astype(np.float64))
    return a == b or (a != a and b != b)


def test_estimate_track_diffusion_with_localization():
    movie, truth = G.simulate_movie(4, 30, 96, 96, 0.3, 4, image_props={"particle_intensity": [300.0, 5.0]}, camera=CAMERA,
                                    generator=torch.Generator().manual_seed(6))
    dm = movie.cuda()
    props = dict(G.DEFAULT_IMAGE_PROPS)
    loc = {"gain": CAMERA["gain"], "offset": CAMERA["offset"], "read_var": (CAMERA["read_noise"] / CAMERA["gain"]) ** 2,
           "sigma0": G.psf_sigma_hr(props) / props["upsampling_factor"]}
    model = _model()
    kw = dict(patch_size=PATCH, dt=DT, batch_size=BATCH, min_track_length=5, max_gap=2)
    base = T.estimate_track_diffusion(dm, model, SEQ_LEN, **kw)
    none = T.estimate_track_diffusion(dm, model, SEQ_LEN, localization=None, **kw)
    res = T.estimate_track_diffusion(dm, model, SEQ_LEN, localization=loc, **kw)
    existing = {"track_id", "length", "n_sequences", "D_model", "D_msd", "D_msd_weighted", "msd", "n_filled"}
    assert set(base) == set(none) == existing and set(res) == existing | {"localization", "sigma2_loc"}
    assert len(base["track_id"]) >= 3
    # the pieces by hand
    table, _ = T.track_particles_tensors(dm, return_dog=False, min_track_length=5, max_gap=2)
    fr, y, x, tid, offsets, filled = T.tracks_table_by_track(table)
    patches = T.extract_patches_flat(dm.float(), fr, y, x, PATCH)
    n_tracks = len(offsets) - 1

    def by_hand(fit):
        msd, d, w = ops.track_msd(torch.stack([fit["y_refined"], fit["x_refined"]], dim=1), offsets.int(), DT, 0)
        return {"D_msd": d, "D_msd_weighted": w, "msd": msd}

    lsq = by_hand(T.refine_localizations_tensors(patches, y, x))
    fit = T.refine_localizations_tensors(patches, y, x, method="mle", camera=loc)
    mle = by_hand(fit)
    for k in ("D_msd", "D_msd_weighted", "msd"):
        assert _bits(base[k], lsq[k]) and _bits(none[k], lsq[k]), k           # localization=None: today's result
        assert _bits(res[k], mle[k]), k                                        # the same estimate on the ML positions
    for k in ("track_id", "length", "n_sequences", "D_model", "n_filled"):     # what does not see the refinement
        assert _bits(base[k], none[k]) and _bits(base[k], res[k]), k
    assert set(res["localization"]) == {"y_std", "x_std", "photons", "background", "psf_size", "deviance", "status"}
    for k, v in res["localization"].items():
        assert v.is_cuda and len(v) == len(fr) and _bits(v, fit[k]), k
    status = fit["status"].cpu().numpy()
    assert (status == 0).mean() > 0.9
    var_row = ((fit["y_std"] ** 2 + fit["x_std"] ** 2) / 2.0).cpu().numpy()
    good = (status == 0) & ~filled.cpu().numpy()
    off = offsets.cpu().numpy()
    want = np.array([var_row[a:b][good[a:b]].mean() if good[a:b].any() else np.nan for a, b in zip(off[:-1], off[1:])])
    got = res["sigma2_loc"].cpu().numpy()
    assert got.shape == (n_tracks,) and np.array_equal(np.isnan(got), np.isnan(want))
    # two orders of an fp64 sum of at most 30 positive terms
    assert np.allclose(got, want, rtol=64 * np.finfo(np.float64).eps, atol=0.0, equal_nan=True)
    # the hidden-Markov fit with the localisation variance taken from the bounds
    sigma2 = float(torch.from_numpy(var_row).cuda()[torch.from_numpy(good).cuda()].mean())
    assert 0.0 < sigma2 < 0.1
    auto = T.estimate_track_diffusion(dm, model, SEQ_LEN, localization=loc, states={"K": 2, "sigma2": "crlb"}, **kw)
    explicit = T.estimate_track_diffusion(dm, model, SEQ_LEN, localization=loc, states={"K": 2, "sigma2": sigma2}, **kw)
    assert auto["states"]["sigma2"] == sigma2                      # the number used is reported only where it was derived
    assert set(auto["states"]) == set(explicit["states"]) | {"sigma2"} and "sigma2" not in explicit["states"]
    for k, v in explicit["states"].items():
        assert _bits(auto["states"][k], v), k
    for k in existing | {"sigma2_loc"}:
        assert _bits(auto[k], res[k]), k
    hand = MSD.fit_diffusion_states(torch.stack([fit["y_refined"], fit["x_refined"]], dim=1), offsets, K=2, dt=DT, sigma2=sigma2)
    assert _bits(hand["Ds"], auto["states"]["Ds"]) and _bits(hand["state"], auto["states"]["state"])
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, states={"K": 2, "sigma2": "crlb"}, **kw)
    with pytest.raises(ValueError, match="refine"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, localization=loc, refine=False, **kw)
