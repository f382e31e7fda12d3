"""GPU: the kernel of csrc/fbm.hip (ops.fgn, mivit_fgn) against the Cholesky oracle of tests/fbm_common.py and the numpy
restatement (helpers/generation._fgn_host), bounds as derived there, and the paths that reach it: fractional_gaussian_noise,
fbm_single_state and simulate_movie on CUDA tensors.  The shapes are the smallest at which the lane striding (T around 64 and
256: one wave, one pass of the 256 threads, two passes), the LDS budget (the T limit) and the row lookup can go wrong."""
import ctypes

import numpy as np
import pytest
import torch

import fbm_common as fc
from moleculardiffusion_mivit_amd.helpers import generation as gen

pytestmark = pytest.mark.gpu


def _kernel(z, alphas):
    out = gen.fractional_gaussian_noise(torch.from_numpy(np.ascontiguousarray(z)).cuda(), alphas)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == z.shape
    return out.cpu().numpy()


@pytest.mark.parametrize("T", [1, 2, 3, 64, 65, 256, 257, 300])
def test_kernel_on_basis_noise_is_the_cholesky_factor(T):
    for alpha in fc.ALPHAS:
        err = fc.basis_error(_kernel(fc.basis(T), alpha), alpha)
        print(f"T {T} alpha {alpha}: |L - chol| = {err:.3g}")
        assert err <= fc.BASIS_ATOL, (T, alpha)


@pytest.mark.parametrize("C", [2, 1, 4])
def test_kernel_on_gaussian_noise_with_mixed_unsorted_exponents(C):
    z, alphas = fc.gaussian(37, 300, C, seed=C), fc.mixed_alphas(37)
    got = _kernel(z, alphas)
    e_chol = float(np.abs(got - fc.oracle(z, alphas)).max())
    e_host = float(np.abs(got - gen.fractional_gaussian_noise(z, alphas)).max())
    print(f"C {C}: |g - chol z| = {e_chol:.3g}, |g - restatement| = {e_host:.3g}")
    assert e_chol <= fc.GAUSS_ATOL and e_host <= fc.GAUSS_ATOL


def test_kernel_at_its_length_limit():
    from moleculardiffusion_mivit_amd import ops
    T = ops.FGN_MAX_T
    z, alphas = fc.gaussian(2, T, 2, seed=11), np.array([1.95, 0.05])
    got = _kernel(z, alphas)
    e_chol = float(np.abs(got - fc.oracle(z, alphas)).max())
    e_host = float(np.abs(got - gen.fractional_gaussian_noise(z, alphas)).max())
    print(f"T {T}: |g - chol z| = {e_chol:.3g}, |g - restatement| = {e_host:.3g}")
    assert e_chol <= fc.GAUSS_ATOL and e_host <= fc.GAUSS_ATOL
    got4 = _kernel(np.concatenate([z, -z], axis=2), alphas)                  # the largest LDS footprint: C = 4
    assert np.array_equal(got4[:, :, :2], got) and np.array_equal(got4[:, :, 2:], -got)
    with pytest.raises(ValueError, match=str(T)):
        gen.fractional_gaussian_noise(torch.zeros(1, T + 1, 2, dtype=torch.float64, device="cuda"), 0.5)
    with pytest.raises(ValueError):
        gen.fractional_gaussian_noise(torch.zeros(1, 8, 5, dtype=torch.float64, device="cuda"), 0.5)


def test_exponent_one_returns_the_noise_bitwise():
    z, alphas = fc.gaussian(6, 300, 2, seed=1), np.array([1.0, 0.5, 1.0, 1.5, 1.0, 1.0])
    got = _kernel(z, alphas)
    ones = alphas == 1.0
    assert np.array_equal(got[ones].view(np.int64), z[ones].view(np.int64))
    assert not np.array_equal(got[~ones], z[~ones])
    z1 = fc.gaussian(3, 1, 2)
    assert np.array_equal(_kernel(z1, 0.3), z1)


def test_kernel_is_deterministic_and_independent_of_the_batch():
    from moleculardiffusion_mivit_amd import _native as N
    n, T, C = 37, 300, 2
    z, alphas = fc.gaussian(n, T, C, seed=12), fc.mixed_alphas(n)
    first = _kernel(z, alphas)
    assert np.array_equal(first.view(np.int64), _kernel(z, alphas).view(np.int64))
    perm = np.random.default_rng(13).permutation(n)
    assert np.array_equal(_kernel(z[perm], alphas[perm]), first[perm])
    for i in (0, 17, n - 1):
        assert np.array_equal(_kernel(z[i:i + 1], alphas[i:i + 1]), first[i:i + 1])
    # through the C-ABI into the middle of one allocation: the rows around the output keep their canary
    canary = -123456.789
    uniq, inv = np.unique(alphas, return_inverse=True)
    gamma = torch.from_numpy(gen.fgn_autocovariance(uniq, T)).cuda()
    rows = torch.from_numpy(inv.astype(np.int32)).cuda()
    zd = torch.from_numpy(z).cuda()
    buf = torch.full((n + 2, T, C), canary, dtype=torch.float64, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    N.check(N.lib.mivit_fgn(vp(zd), vp(gamma), vp(rows), n, T, C, len(uniq), vp(buf[1:]),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mivit_fgn")
    back = buf.cpu().numpy()
    assert bool((back[0] == canary).all()) and bool((back[-1] == canary).all())
    assert np.array_equal(back[1:-1], first)
    assert np.array_equal(zd.cpu().numpy(), z)                               # the input is not written


def test_empty_inputs_do_not_launch():
    for shape in ((0, 300, 2), (5, 0, 2), (0, 0, 1)):
        out = gen.fractional_gaussian_noise(torch.zeros(shape, dtype=torch.float64, device="cuda"), 0.5)
        assert out.is_cuda and tuple(out.shape) == shape
    torch.cuda.synchronize()


@pytest.mark.parametrize("Ds", [(0.7, 0.0), (0.7, 0.05)])
def test_fbm_single_state_on_the_gpu_at_one_is_brownian_single_state_bitwise(Ds):
    g = lambda: torch.Generator(device="cuda").manual_seed(3)      # noqa: E731
    want = gen.brownian_single_state(11, 40, Ds, dt=0.5, generator=g(), device="cuda")
    got = gen.fbm_single_state(11, 40, Ds, alphas=1, dt=0.5, generator=g(), device="cuda")
    for w, h in zip(want, got):
        assert h.is_cuda and w.dtype == h.dtype and torch.equal(w, h)
    assert np.array_equal(want[0].cpu().numpy().view(np.int32), got[0].cpu().numpy().view(np.int32))


def test_ensemble_msd_follows_the_power_law_on_the_gpu():
    """the law of tests/test_fbm.py::test_ensemble_msd_follows_the_power_law, once through the kernel: 8192 chi^2_1 samples,
    relative sigma 1.56 %, bound 6 sigma = 9.4 %; two exponents in one launch"""
    D, dt, n = 0.3, 0.5, 4096
    alphas = torch.cat([torch.full((n,), 0.5), torch.full((n,), 1.5)])
    trajs, labels = gen.fbm_single_state(2 * n, 64, (D, 0.0), alphas=alphas, dt=dt,
                                         generator=torch.Generator(device="cuda").manual_seed(7), device="cuda")
    assert trajs.is_cuda and torch.equal(labels[0, :, 0].cpu(), alphas)
    trajs = trajs.cpu().numpy()
    for half, alpha in ((slice(0, n), 0.5), (slice(n, 2 * n), 1.5)):
        err = fc.ensemble_msd_error(trajs[:, half], D, dt, alpha)
        print(f"alpha {alpha}: worst relative MSD gap {err:.3%}")
        assert err <= 0.094


def _movie(alphas, seed=8):
    props = {"upsampling_factor": 3}
    return gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, image_props=props,
                              generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda", alphas=alphas)


def test_simulate_movie_on_the_gpu():
    movie0, truth0 = _movie(None)
    movie1, truth1 = _movie(torch.ones(5))
    assert movie1.is_cuda and set(truth1) == set(truth0) | {"alpha"}
    assert torch.equal(movie0, movie1)
    for k, v in truth0.items():
        assert v.dtype == truth1[k].dtype and torch.equal(v, truth1[k]), k
    assert torch.equal(truth1["alpha"].cpu(), torch.ones(5, dtype=torch.float64))
    movie, truth = _movie(0.5)
    assert bool(torch.isfinite(truth["pos"]).all()) and bool(torch.isfinite(movie).all())
    assert not torch.equal(truth["pos"], truth0["pos"]) and truth["alpha"].is_cuda
