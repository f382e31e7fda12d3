"""The oracle and the shared cases of tests/test_fbm.py (CPU) and tests/test_fbm_gpu.py: fractional Gaussian noise by
DEFINITION, np.linalg.cholesky of the T x T Toeplitz matrix of the autocovariance applied to z in float64, not a second
implementation of the recursion.

Bounds (float64 Durbin-Levinson against this oracle, alpha in {0.05, 0.1, 0.5, 1, 1.5, 1.9, 1.95}, measured on the CPU):
  basis noise (z = identity, the output is L itself; its entries are <= 1 in magnitude): worst |L - chol| 6.5e-15 at T = 300,
    1.14e-14 at T = 2048 (alpha = 1.95)                                                      -> BASIS_ATOL = 1e-12 (about 90x)
  Gaussian noise (|g| <= 5): worst |g - chol z| 6.3e-14 at T = 300, 3.7e-13 at T = 2048      -> GAUSS_ATOL = 1e-10 (about 270x)
  reversing every sum of the recursion moves the result by 2.4e-14 (T = 300) / 8.1e-14 (T = 2048): the only way the kernel
  and the numpy restatement may differ.
The restatement and the kernel take all three sums of a step on the previous step's coefficients (one reduction per step);
the gap of THAT formula to the oracle is re-measured in the docstring of tests/test_fbm.py."""
import functools

import numpy as np

from moleculardiffusion_mivit_amd.helpers import generation as gen

BASIS_ATOL = 1e-12
GAUSS_ATOL = 1e-10
ALPHAS = (0.05, 0.5, 1.0, 1.5, 1.95)
# mixed and unsorted, with repeats: equal exponents share a row of gamma
MIXED_ALPHAS = (1.5, 0.05, 1.0, 1.95, 0.5, 0.5, 1.9, 0.1, 1.5, 1.0, 0.7)


@functools.lru_cache(maxsize=None)
def cholesky_factor(alpha: float, T: int) -> np.ndarray:
    """L [T, T] float64 (read-only), L L^T = Toeplitz(gamma(alpha))."""
    gam = gen.fgn_autocovariance(alpha, T)[0]
    idx = np.abs(np.arange(T)[:, None] - np.arange(T)[None, :])
    L = np.linalg.cholesky(gam[idx])
    L.setflags(write=False)
    return L


def oracle(z: np.ndarray, alphas) -> np.ndarray:
    """z [N, T, C] float64, alphas [N] -> L(alpha_n) z[n] per trajectory."""
    z = np.asarray(z, np.float64)
    alphas = np.broadcast_to(np.asarray(alphas, np.float64), (z.shape[0],))
    out = np.empty_like(z)
    for n in range(z.shape[0]):
        out[n] = cholesky_factor(float(alphas[n]), z.shape[1]) @ z[n]
    return out


def mixed_alphas(n: int) -> np.ndarray:
    return np.array([MIXED_ALPHAS[i % len(MIXED_ALPHAS)] for i in range(n)], np.float64)


def gaussian(n: int, T: int, C: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((n, T, C))


def basis(T: int) -> np.ndarray:
    """z [T, T, 2]: trajectory i holds the i-th unit vector on axis 0 and its negative on axis 1, so the output of trajectory
    i is column i of L (and its negative)."""
    z = np.zeros((T, T, 2))
    z[np.arange(T), np.arange(T), 0] = 1.0
    z[np.arange(T), np.arange(T), 1] = -1.0
    return z


def basis_error(got: np.ndarray, alpha: float) -> float:
    """max |got - L| over both axes for got = fGn(basis(T))."""
    L = cholesky_factor(float(alpha), got.shape[0])
    return max(float(np.abs(got[:, :, 0].T - L).max()), float(np.abs(got[:, :, 1].T + L).max()))


def ensemble_msd_error(trajs, D: float, dt: float, alpha: float, lags=(1, 4, 16, 63)) -> float:
    """worst relative gap of the per-axis ensemble MSD <(x(k) - x(0))^2> of trajs [T, N, 2] to 2 D dt k^alpha."""
    x = np.asarray(trajs, np.float64)
    worst = 0.0
    for k in lags:
        want = 2.0 * D * dt * k ** alpha
        worst = max(worst, abs(float(((x[k] - x[0]) ** 2).mean()) / want - 1.0))
    return worst
