"""CPU: anomalous diffusion (helpers/generation.fractional_gaussian_noise, fbm_single_state, simulate_movie(alphas=...),
helpers/msd.estimate_alpha) and the argument checks of mivit_fgn (csrc/fbm.hip), which precede every HIP call.

The numpy restatement takes the three sums of a step on the previous step's coefficients, as the kernel does (one
reduction per step).  Its gap to the Cholesky oracle of tests/fbm_common.py, measured on the CPU for alpha in {0.05, 0.1, 0.5,
1, 1.5, 1.9, 1.95}:
  basis noise    T = 300: 5.9e-15 (alpha 1.95)    T = 2048: 1.14e-14 (alpha 1.95)    bound 1e-12
  Gaussian noise T = 300: 6.7e-14 (alpha 1.95)    T = 2048: 3.5e-13 (alpha 1.95)     bound 1e-10
and the identity, exactly, at alpha = 1 for every T tried: the same as the two-reduction recursion the bounds were set from."""
import ctypes

import numpy as np
import pytest
import torch

import fbm_common as fc
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as MSD


@pytest.mark.parametrize("T", [1, 2, 3, 64, 300])
@pytest.mark.parametrize("alpha", fc.ALPHAS)
def test_restatement_on_basis_noise_is_the_cholesky_factor(T, alpha):
    got = gen.fractional_gaussian_noise(fc.basis(T), alpha)
    assert got.shape == (T, T, 2) and got.dtype == np.float64
    err = fc.basis_error(got, alpha)
    print(f"T {T} alpha {alpha}: |L - chol| = {err:.3g}")
    assert err <= fc.BASIS_ATOL


def test_restatement_on_gaussian_noise_with_mixed_unsorted_exponents():
    z, alphas = fc.gaussian(8, 300, 2), fc.mixed_alphas(8)
    assert not np.all(np.diff(alphas) >= 0) and len(set(alphas)) < 8 < 2 * len(set(alphas))
    got = gen.fractional_gaussian_noise(z, alphas)
    err = float(np.abs(got - fc.oracle(z, alphas)).max())
    print(f"|g - chol z| = {err:.3g}")
    assert err <= fc.GAUSS_ATOL
    # tensors in, tensors out, the same numbers; a [N] tensor of exponents as well
    t = gen.fractional_gaussian_noise(torch.from_numpy(z), torch.from_numpy(alphas))
    assert torch.is_tensor(t) and t.dtype == torch.float64 and np.array_equal(t.numpy(), got)
    # float32 noise is widened, the result is float64
    assert gen.fractional_gaussian_noise(torch.from_numpy(z).float(), 0.5).dtype == torch.float64


def test_exponent_one_returns_the_noise_bitwise():
    z, alphas = fc.gaussian(6, 300, 2, seed=1), np.array([1.0, 0.5, 1.0, 1.5, 1.0, 1.0])
    got = gen.fractional_gaussian_noise(z, alphas)
    ones = alphas == 1.0
    assert np.array_equal(got[ones].view(np.int64), z[ones].view(np.int64))
    assert not np.array_equal(got[~ones], z[~ones])
    assert np.array_equal(gen.fgn_autocovariance(1.0, 300)[0], np.eye(300)[0])
    for T in (0, 1):                                             # nothing to correlate
        z = fc.gaussian(3, T, 2)
        assert np.array_equal(gen.fractional_gaussian_noise(z, 0.3), z)


@pytest.mark.parametrize("Ds", [(0.7, 0.0), (0.7, 0.05)])
def test_fbm_single_state_at_one_is_brownian_single_state_bitwise(Ds):
    want = gen.brownian_single_state(11, 40, Ds, dt=0.5, generator=torch.Generator().manual_seed(3))
    got = gen.fbm_single_state(11, 40, Ds, alphas=1, dt=0.5, generator=torch.Generator().manual_seed(3))
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and torch.equal(w, g)
    assert np.array_equal(want[0].numpy().view(np.int32), got[0].numpy().view(np.int32))


def test_brownian_single_state_forwards_other_exponents():
    want = gen.fbm_single_state(5, 30, (1.0, 0.1), alphas=0.5, generator=torch.Generator().manual_seed(4))
    got = gen.brownian_single_state(5, 30, (1.0, 0.1), alphas=0.5, generator=torch.Generator().manual_seed(4))
    plain = gen.brownian_single_state(5, 30, (1.0, 0.1), generator=torch.Generator().manual_seed(4))
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert bool((got[1][..., 0] == 0.5).all()) and torch.equal(got[1][..., 1], plain[1][..., 1])
    assert not torch.equal(got[0], plain[0]) and torch.equal(got[0][:2], plain[0][:2])     # the first increment is z itself


def test_fbm_single_state_shapes_labels_and_exponent_draws():
    N, T = 64, 12
    trajs, labels = gen.fbm_single_state(N, T, (2.0, 0.0), alphas=(1.0, 0.5), generator=torch.Generator().manual_seed(5))
    assert trajs.shape == (T, N, 2) and labels.shape == (T, N, 3) and trajs.dtype == labels.dtype == torch.float32
    assert bool((trajs[0] == 0).all()) and bool(torch.isfinite(trajs).all())
    a = labels[0, :, 0]
    assert bool((labels[..., 0] == a).all()) and bool((labels[..., 1] == 2.0).all()) and bool((labels[..., 2] == 0).all())
    assert bool(((a >= np.float32(gen.ALPHA_MIN)) & (a <= np.float32(gen.ALPHA_MAX))).all())
    assert len(torch.unique(a)) > N // 2 and float(a.std()) > 0.3              # var 0.5 with redraws: really drawn per particle
    # per-particle exponents as given, in a tensor or an array; a pair without variance draws nothing
    given = torch.linspace(0.1, 1.9, N)
    _, lab = gen.fbm_single_state(N, T, alphas=given, generator=torch.Generator().manual_seed(5))
    assert torch.equal(lab[3, :, 0], given)
    t1, _ = gen.fbm_single_state(N, T, alphas=(0.8, 0.0), generator=torch.Generator().manual_seed(6))
    t2, _ = gen.fbm_single_state(N, T, alphas=np.full(N, 0.8), generator=torch.Generator().manual_seed(6))
    assert torch.equal(t1, t2)
    for bad in (0.0, gen.ALPHA_MIN - 1e-3, gen.ALPHA_MAX + 1e-3, 2.0, float("nan"), torch.full((N,), 2.5), (2.5, 0.1),
                torch.ones(N + 1)):
        with pytest.raises(ValueError):
            gen.fbm_single_state(N, T, alphas=bad)
    with pytest.raises(ValueError):
        gen.brownian_single_state(N, T, alphas=2.0)
    with pytest.raises(ValueError):
        gen.fractional_gaussian_noise(np.zeros((2, 5, 2)), [0.5, 1.99])
    with pytest.raises(ValueError):
        gen.fractional_gaussian_noise(np.zeros((2, 5)), 0.5)


@pytest.mark.parametrize("alpha", [0.5, 1.5])
def test_ensemble_msd_follows_the_power_law(alpha):
    """<x^2(k)> per axis = 2 D dt k^alpha: the mean of 4096 x 2 = 8192 chi^2_1 samples, relative sigma sqrt(2 / 8192) = 1.56 %;
    the bound is 6 sigma = 9.4 %."""
    D, dt = 0.3, 0.5
    trajs, _ = gen.fbm_single_state(4096, 64, (D, 0.0), alphas=alpha, dt=dt, generator=torch.Generator().manual_seed(7))
    err = fc.ensemble_msd_error(trajs.numpy(), D, dt, alpha)
    print(f"alpha {alpha}: worst relative MSD gap {err:.3%}")
    assert err <= 0.094


def _movie(alphas, seed=8, **kw):
    props = {"upsampling_factor": 3}
    return gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, image_props=props, generator=torch.Generator().manual_seed(seed),
                              alphas=alphas, **kw)


def test_simulate_movie_with_unit_exponents_is_the_brownian_movie_bitwise():
    movie0, truth0 = _movie(None)
    movie1, truth1 = _movie(torch.ones(5))
    assert "alpha" not in truth0 and set(truth1) == set(truth0) | {"alpha"}
    assert torch.equal(movie0, movie1)
    for k, v in truth0.items():
        assert v.dtype == truth1[k].dtype and torch.equal(v, truth1[k]), k
    assert truth1["alpha"].dtype == torch.float64 and torch.equal(truth1["alpha"], torch.ones(5, dtype=torch.float64))


def test_simulate_movie_with_exponents():
    given = torch.tensor([0.3, 1.0, 1.7, 0.3, 0.9])
    movie, truth = _movie(given, blink=0.2)
    assert torch.equal(truth["alpha"], given.double()) and "visible" in truth
    assert movie.shape == (6, 40, 48) and bool(torch.isfinite(movie).all()) and bool(torch.isfinite(truth["pos"]).all())
    _, brown = _movie(None, blink=0.2)
    assert not torch.equal(truth["pos"][0], brown["pos"][0]) and torch.equal(truth["pos"][1], brown["pos"][1])
    _, drawn = _movie((1.0, 0.2))
    assert drawn["alpha"].shape == (5,) and len(torch.unique(drawn["alpha"])) == 5
    assert bool(((drawn["alpha"] >= gen.ALPHA_MIN) & (drawn["alpha"] <= gen.ALPHA_MAX)).all())
    _, same = _movie(0.6)
    assert torch.equal(same["alpha"], torch.full((5,), 0.6, dtype=torch.float64))
    for bad in (2.0, 0.0, torch.tensor([0.5, 0.5, 0.5, 0.5, 1.99]), torch.ones(4), (3.0, 0.1)):
        with pytest.raises(ValueError):
            _movie(bad)


def test_simulate_movie_keeps_the_msd_per_frame():
    """sub-steps are fGn(z) * sqrt(2 D / npos^alpha), so that the npos sub-steps of a frame add up to a per-axis MSD of 2 D and
    k frames to 2 D k^alpha.  Checked exactly, not statistically: the draws are replayed in their order (a number for D draws
    nothing; rand(Np, 2) for the start; randn(Np, T, 2)) and the positions rebuilt in float64.  simulate_movie holds steps and
    positions in float32: 24 steps of rounding 6e-8 relative on positions below 16 pixels stay under 1e-4."""
    D, npos, F = 0.5, 8, 3
    given = torch.tensor([0.5, 1.0, 1.6, 0.05, 1.95], dtype=torch.float64)
    props = {"upsampling_factor": 1, "particle_intensity": [0, 0], "background_intensity": [0, 0], "poisson_noise": -1}
    _, truth = gen.simulate_movie(5, F, 16, 16, D, npos, image_props=props, margin=0.0,
                                  generator=torch.Generator().manual_seed(9), alphas=given)
    g = torch.Generator().manual_seed(9)
    start = torch.rand(5, 2, generator=g) * torch.tensor([15.0, 15.0])
    z = torch.randn(5, F * npos, 2, generator=g).double()
    steps = gen.fractional_gaussian_noise(z, given) * torch.sqrt(2.0 * D / npos ** given).view(5, 1, 1)
    steps[:, 0] = 0.0
    want = start.double().view(5, 1, 2) + torch.cumsum(steps, dim=1)
    assert float((truth["pos"].double() - want).abs().max()) <= 1e-4
    # and the law itself from the factor: Var(sum of k npos unit fGn steps) = (k npos)^alpha, times 2 D / npos^alpha = 2 D k^alpha
    for alpha in (0.5, 1.6):
        for k in (1, 3):
            L = fc.cholesky_factor(alpha, k * npos)
            var = float((L.sum(axis=0) ** 2).sum()) * 2 * D / npos ** alpha
            assert abs(var / (2 * D * k ** alpha) - 1.0) <= 1e-12


def test_estimate_alpha():
    lag = np.arange(0, 40, dtype=np.float64)
    alphas = np.array([0.3, 1.0, 1.7])
    msds = 0.8 * lag[None, :] ** alphas[:, None]
    got = MSD.estimate_alpha(msds)
    assert isinstance(got, np.ndarray) and np.abs(got - alphas).max() <= 1e-12
    assert np.abs(MSD.estimate_alpha(msds, max_lag=5) - alphas).max() <= 1e-12
    t = MSD.estimate_alpha(torch.from_numpy(msds), max_lag=1000)
    assert torch.is_tensor(t) and t.dtype == torch.float64 and np.abs(t.numpy() - alphas).max() <= 1e-12
    # short tracks: the zero padding of track_msd's rows is skipped, fewer than two usable lags give NaN
    rows = msds.copy()
    rows[0, 3:] = 0.0                                            # a track of 3 rows: lags 1 and 2
    rows[1, 2:] = 0.0                                            # one lag
    rows[2, :] = 0.0                                             # none
    got = MSD.estimate_alpha(rows)
    assert abs(got[0] - 0.3) <= 1e-12 and np.isnan(got[1]) and np.isnan(got[2])
    # non-positive lags inside a row are skipped, not fatal
    rows = msds.copy()
    rows[:, 4], rows[:, 9], rows[0, 11] = 0.0, -1.0, np.nan
    assert np.abs(MSD.estimate_alpha(rows) - alphas).max() <= 1e-12
    # the rows of track_msd as they come
    trajs, _ = gen.fbm_single_state(3, 50, alphas=0.5, generator=torch.Generator().manual_seed(10))
    pos = trajs.permute(1, 0, 2).reshape(-1, 2).double()
    curves, _, _ = MSD.track_msd(pos, torch.tensor([0, 50, 100, 150]))
    assert MSD.estimate_alpha(curves, max_lag=10).shape == (3,)
    assert MSD.estimate_alpha(np.zeros((0, 7))).shape == (0,)
    with pytest.raises(ValueError):
        MSD.estimate_alpha(np.zeros(7))
    with pytest.raises(ValueError):
        MSD.estimate_alpha(msds, max_lag=0)


def test_mivit_fgn_rejects_bad_arguments_without_crashing():
    """Null pointers, negative sizes, C out of range and T over the limit come back as an error string: every check precedes
    the first HIP call, so this runs where no GPU is.  N = 0 and T = 0 are no-ops."""
    from moleculardiffusion_mivit_amd import _native as N
    from moleculardiffusion_mivit_amd import ops
    fake = ctypes.c_void_p(0x1000)                               # never dereferenced
    fgn = N.lib.mivit_fgn
    assert fgn(fake, fake, fake, 0, 300, 2, 1, fake, None) == 0
    assert fgn(fake, fake, fake, 7, 0, 2, 1, fake, None) == 0
    assert fgn(None, None, None, 0, 0, 1, 0, None, None) == 0
    for args, word in (((None, fake, fake, 3, 8, 2, 1, fake), "null"), ((fake, None, fake, 3, 8, 2, 1, fake), "null"),
                       ((fake, fake, None, 3, 8, 2, 1, fake), "null"), ((fake, fake, fake, 3, 8, 2, 1, None), "null"),
                       ((fake, fake, fake, -1, 8, 2, 1, fake), "negative"), ((fake, fake, fake, 3, -8, 2, 1, fake), "negative"),
                       ((fake, fake, fake, 3, 8, 2, -1, fake), "negative"), ((fake, fake, fake, 3, 8, 2, 0, fake), "row"),
                       ((fake, fake, fake, 3, 8, 5, 1, fake), "axes"), ((fake, fake, fake, 3, 8, 0, 1, fake), "axes"),
                       ((fake, fake, fake, 3, ops.FGN_MAX_T + 1, 2, 1, fake), "limit"),
                       ((fake, fake, fake, 0, ops.FGN_MAX_T + 1, 2, 1, fake), "limit")):
        rc = fgn(*args, None)
        assert rc != 0 and word in N.last_error(), (args, N.last_error())
        with pytest.raises(N.MivitError):
            N.check(rc, "mivit_fgn")
    assert str(ops.FGN_MAX_T) in N.last_error() and ops.FGN_MAX_T >= 2048 and ops.FGN_MAX_C == 4
