"""Synthetic single-molecule data for the training loops (the step right before the hot path).

Own, vectorised, seedable restatement of what the reference's generator produces, written with torch ops so it runs
on the host or directly on the GPU (no andi_datasets / skimage dependency):

* ``brownian_single_state``  stands in for ``andi_datasets.models_phenom().single_state(N, L=0, T, Ds=[mean, var],
  alphas=1)`` as consumed at ``Experiments/PSFNoise/trainModelsPSFNoise.py:128-142``: free Brownian motion,
  increments ``sqrt(2 D dt) N(0,1)`` (the law spelled out in ``mitochondria_simulation/mitochnodria.py:470-474``),
  per-particle ``D ~ N(mean, var)`` redrawn until positive; returns ``(T, N, 2)`` trajectories and ``(T, N, 3)``
  labels ``[alpha, D, state]``.
* ``fbm_single_state`` / ``fractional_gaussian_noise``: the same with an anomalous exponent, ``single_state(..., alphas=a)``:
  exact fractional Gaussian noise by the Durbin-Levinson recursion, csrc/fbm.hip for GPU tensors, numpy otherwise.
* ``render_frames`` is the noiseless image model of ``helpers/helpersGeneration.py:283-308`` /
  ``trainSettingsPSFNoise.py:265-292``: each frame is the sum of ``nPosPerFrame`` peak-normalised Gaussian spots on a
  ``upsampling_factor``-times finer grid, mean-pooled back.  A peak-normalised 2-D Gaussian on a grid is an outer
  product of two 1-D profiles, and mean-pooling an outer product is the outer product of the pooled profiles, so a
  frame costs O(p * (G + P^2)) instead of O(p * G^2) and the Python triple loop disappears.
* noise models: clipped-Gaussian background + Poisson, in both variants the reference uses.
* ``normalize_images`` = ``helpersGeneration.py:356-400``.
* the Denoising experiment's data (``helpersGeneration.py:422-660``): ``trajectories_to_video_multiple_settings`` (no
  noise / background / Poisson / Gaussian-filtered Poisson), Richardson-Lucy deconvolution with total-variation
  regularisation (``richardson_lucy_tv*``, ``apply_rl_tv_tensor*``, ``tv_gradient``, ``create_gaussian_psf``) and
  ``trajs_to_vid_norm_rl``.  GPU tensors go to csrc/deconv.hip; numpy / CPU input to a numpy restatement vectorised over
  frames that sums in the kernel's order (bitwise the kernel's result; within FFT rounding of the reference's).
* whole fields of view with known truth (no counterpart in the reference, whose real movies carry none): ``render_movie``
  (the same image model for many particles in one [F, H, W] movie; GPU tensors go to csrc/movie.hip, anything else to a
  float64 restatement) and ``simulate_movie`` (Brownian particles, lifetimes, background, Poisson gain, and the truth table
  ``helpers/tracking.score_tracking`` scores a detections table against).

The reference draws from the unseeded global numpy RNG, so agreement is distributional; the deterministic part
(noise-free rendering) is pinned against a naive per-pixel loop in ``tests/test_generation.py``.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

DEFAULT_IMAGE_PROPS = {
    "particle_intensity": [500, 20],
    "NA": 1.46,
    "wavelength": 500e-9,
    "psf_division_factor": 1,
    "resolution": 100e-9,
    "output_size": 32,
    "upsampling_factor": 5,
    "background_intensity": [100, 10],
    "poisson_noise": 100,
    "trajectory_unit": 100,
}


def _as_tensor(x, device=None, dtype=torch.float32):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype)
    return torch.as_tensor(x, dtype=dtype, device=device)


def brownian_single_state(N: int, T: int, Ds=(1.0, 0.0), alphas: float = 1.0, dt: float = 1.0,
                          generator: Optional[torch.Generator] = None, device="cpu"):
    """(T, N, 2) trajectories and (T, N, 3) labels [alpha, D, state=0] of freely diffusing particles.  Any alphas other than
    the number 1 is anomalous diffusion: fbm_single_state."""
    if not (isinstance(alphas, (int, float)) and not isinstance(alphas, bool) and float(alphas) == 1.0):
        return fbm_single_state(N, T, Ds, alphas, dt, generator, device)
    mean, var = float(Ds[0]), float(Ds[1])
    D = torch.full((N,), mean, device=device)
    if var > 0:
        D = mean + math.sqrt(var) * torch.randn(N, generator=generator, device=device)
        for _ in range(64):                      # redraw non-positive coefficients (AnDi constrains D > 0)
            bad = D <= 1e-4
            if not bool(bad.any()):
                break
            D = torch.where(bad, mean + math.sqrt(var) * torch.randn(N, generator=generator, device=device), D)
        D = D.clamp_min(1e-4)
    steps = torch.randn(T, N, 2, generator=generator, device=device) * torch.sqrt(2.0 * D * dt).view(1, N, 1)
    steps[0] = 0.0
    trajs = torch.cumsum(steps, dim=0)
    labels = torch.stack([torch.full((T, N), float(alphas), device=device), D.view(1, N).expand(T, N),
                          torch.zeros(T, N, device=device)], dim=-1)
    return trajs, labels


def _velocity_matrix(velocity, n: int) -> torch.Tensor:
    """velocity, (vy, vx) as [2] or one per particle [n, 2], as a float64 CPU tensor [n, 2] of finite numbers (ValueError
    otherwise)."""
    what = f"velocity must be a real (vy, vx) pair or [{n}, 2] values"
    try:
        v = (velocity if torch.is_tensor(velocity) else torch.from_numpy(np.array(velocity))).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}, got {velocity!r}") from None
    if v.dtype == torch.bool or v.is_complex() or tuple(v.shape) not in ((2,), (n, 2)):
        raise ValueError(f"{what}, got {v.dtype} {tuple(v.shape)}")
    v = v.double()
    if not bool(torch.isfinite(v).all()):
        raise ValueError("velocity must be finite")
    return (v.view(1, 2).expand(n, 2) if v.dim() == 1 else v).contiguous()


def directed_single_state(N: int, T: int, Ds=(1.0, 0.0), velocity=(0.0, 0.0), dt: float = 1.0,
                          generator: Optional[torch.Generator] = None, device="cpu"):
    """(T, N, 2) trajectories and (T, N, 3) labels [alpha = 1, D, state = 0] of directed motion: diffusion plus a constant
    velocity, (vy, vx) as [2] or one per particle [N, 2], in units of length per unit of dt.  It draws exactly what
    brownian_single_state draws and adds velocity * t * dt at step t (in float64, rounded once): a zero velocity gives its
    trajectories bit for bit.  What helpers/msd.estimate_directed_ml estimates."""
    vel = _velocity_matrix(velocity, N)
    trajs, labels = brownian_single_state(N, T, Ds, 1.0, dt, generator, device)
    t = torch.arange(T, dtype=torch.float64, device=trajs.device) * float(dt)
    return (trajs.double() + t.view(T, 1, 1) * vel.to(trajs.device).view(1, N, 2)).to(trajs.dtype), labels


def _radius_vector(radius, n: int) -> torch.Tensor:
    """radius, a number or [n] values, as a float64 CPU tensor [n] of positive finite numbers (ValueError otherwise)."""
    try:
        r = (radius.detach().to("cpu", torch.float64) if torch.is_tensor(radius) else torch.as_tensor(np.asarray(radius, dtype=np.float64))).reshape(-1)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"radius must be a number or hold one radius per particle ({n}), got {radius!r}") from None
    if r.numel() == 1:
        r = r.expand(n)
    if r.numel() != n:
        raise ValueError(f"radius must be a number or hold one radius per particle ({n}), got {r.numel()}")
    if n and not bool(((r > 0) & torch.isfinite(r)).all()):
        raise ValueError("radius must be positive and finite")
    return r.contiguous()


def _ou_walk(z: torch.Tensor, D: torch.Tensor, radius: torch.Tensor, dt: float, stationary: bool) -> torch.Tensor:
    """The exact discretisation of an isotropic Ornstein-Uhlenbeck process about 0 from standard normals z [T, N, 2] (float64):
    stationary variance per axis s2 = radius^2 / 2, rate lam = D / s2, phi = exp(-lam dt); x_t = phi x_{t-1} + sqrt(s2 (1 -
    phi^2)) z_t, with sqrt(s2 (1 - phi^2)) = sqrt(-s2 expm1(-2 lam dt)).  x_0 = sqrt(s2) z_0, the stationary law, or 0 (the
    centre).  D, radius [N] float64 on z's device -> [T, N, 2] float64.  A plain loop over the steps, vectorised over the
    particles."""
    s2 = 0.5 * radius * radius
    lam = D / s2
    phi = torch.exp(-lam * dt).view(-1, 1)
    amp = torch.sqrt(-s2 * torch.expm1(-2.0 * lam * dt)).view(-1, 1)
    x = torch.empty_like(z)
    if z.shape[0]:
        x[0] = torch.sqrt(s2).view(-1, 1) * z[0] if stationary else 0.0
    for t in range(1, z.shape[0]):
        x[t] = phi * x[t - 1] + amp * z[t]
    return x


def confined_single_state(N: int, T: int, Ds=(1.0, 0.0), radius=1.0, dt: float = 1.0,
                          generator: Optional[torch.Generator] = None, device="cpu"):
    """(T, N, 2) trajectories and (T, N, 3) labels [alpha = 1, D, state = 0] of particles that diffuse in a harmonic well about
    the origin: an isotropic Ornstein-Uhlenbeck process by its exact discretisation (_ou_walk), so the statistics hold at any
    dt.  radius, a number or [N] values, is the RMS distance from the centre in 2-D, sqrt(2 s2) with the stationary variance s2
    per axis; the rate at which a particle is pulled back is D / s2.  Draws, in this order: D exactly as
    brownian_single_state draws it, then randn(T, N, 2) where the Brownian steps are; row 0, which the free walk throws away,
    places the particle in the stationary law.  As radius -> inf the steps are those of brownian_single_state.  The model of
    helpers/msd.estimate_confinement_ml."""
    mean, var = float(Ds[0]), float(Ds[1])
    rad = _radius_vector(radius, N).to(device)
    D = torch.full((N,), mean, device=device)
    if var > 0:
        D = mean + math.sqrt(var) * torch.randn(N, generator=generator, device=device)
        for _ in range(64):                      # redraw non-positive coefficients, as brownian_single_state
            bad = D <= 1e-4
            if not bool(bad.any()):
                break
            D = torch.where(bad, mean + math.sqrt(var) * torch.randn(N, generator=generator, device=device), D)
        D = D.clamp_min(1e-4)
    z = torch.randn(T, N, 2, generator=generator, device=device)
    trajs = _ou_walk(z.double(), D.double(), rad, float(dt), True).float()
    labels = torch.stack([torch.ones(T, N, device=device), D.view(1, N).expand(T, N), torch.zeros(T, N, device=device)], dim=-1)
    return trajs, labels


# ------------------------------------------------------------------------------------------------------------------------
# Anomalous diffusion: fractional Brownian motion, MSD = 2 D dt k^alpha per axis (csrc/fbm.hip)
# ------------------------------------------------------------------------------------------------------------------------
ALPHA_MIN = 0.05             # the Toeplitz matrix of the autocovariance gets ill-conditioned towards alpha = 2; the accuracy of
ALPHA_MAX = 1.95             # the recursion against Cholesky (tests/test_fbm.py) was measured on this range


def fgn_autocovariance(alphas, T: int) -> np.ndarray:
    """gamma [U, T] float64 of unit-variance fractional Gaussian noise, one row per exponent (Hurst H = alpha / 2):
    gamma[k] = (|k + 1|^alpha - 2 |k|^alpha + |k - 1|^alpha) / 2, gamma[0] = 1.  THE function both the kernel and the host
    restatement take gamma from.  At alpha = 1 every entry past the first is exactly 0."""
    a = np.atleast_1d(np.asarray(alphas, dtype=np.float64)).reshape(-1, 1)
    k = np.arange(int(T), dtype=np.float64).reshape(1, -1)
    return 0.5 * (np.power(k + 1.0, a) - 2.0 * np.power(k, a) + np.power(np.abs(k - 1.0), a))


def _fgn_host(z: np.ndarray, gam: np.ndarray) -> np.ndarray:
    """The recursion of csrc/fbm.hip in numpy, vectorised over trajectories: z [N, T, C], gam [N, T] float64 -> g [N, T, C].
    Durbin-Levinson with the three sums of step n taken on the coefficients of step n - 1 (include/mivit_hip.h, mivit_fgn);
    differs from the kernel in the order of the sums only."""
    N, T, C = z.shape
    g = np.empty((N, T, C), np.float64)
    if N == 0 or T == 0:
        return g
    phi = np.zeros((N, T), np.float64)
    v = gam[:, 0].copy()
    g[:, 0] = np.sqrt(v)[:, None] * z[:, 0]
    for n in range(1, T):
        p, pr = phi[:, 1:n], phi[:, n - 1:0:-1]                            # phi[j], phi[n - j], j = 1 .. n - 1
        gv = g[:, n - 1:0:-1]                                              # g[n - j]
        A = (p * gam[:, n - 1:0:-1]).sum(axis=1)
        B = (p[:, :, None] * gv).sum(axis=1)
        R = (pr[:, :, None] * gv).sum(axis=1)
        kappa = (gam[:, n] - A) / v
        v = v * (1.0 - kappa * kappa)
        k1 = kappa[:, None]
        g[:, n] = ((B - k1 * R) + k1 * g[:, 0]) + np.sqrt(v)[:, None] * z[:, n]
        phi[:, 1:n] = p - k1 * pr                                          # the right side is a new array: no aliasing
        phi[:, n] = kappa
    return g


def _alpha_vector(alphas, n: int) -> torch.Tensor:
    """alphas, a number or [n] values, as a float64 CPU tensor [n] inside [ALPHA_MIN, ALPHA_MAX] (ValueError otherwise)."""
    if torch.is_tensor(alphas):
        a = alphas.detach().to("cpu", torch.float64).reshape(-1)
    else:
        a = torch.as_tensor(np.asarray(alphas, dtype=np.float64)).reshape(-1)
    if a.numel() == 1 and n != 1:
        a = a.expand(n).clone()
    if a.numel() != n:
        raise ValueError(f"alphas must be a number or hold one exponent per trajectory ({n}), got {a.numel()}")
    if n and not bool(((a >= ALPHA_MIN) & (a <= ALPHA_MAX)).all()):        # NaN fails both comparisons
        raise ValueError(f"alphas must lie in [{ALPHA_MIN}, {ALPHA_MAX}] (ALPHA_MIN, ALPHA_MAX), got {float(a.min())} .. "
                         f"{float(a.max())}")
    return a


def fractional_gaussian_noise(z, alphas):
    """Unit-variance fractional Gaussian noise from standard normals: z [N, T, C], alphas a number or [N] (one exponent per
    trajectory, shared by its C axes) -> float64 of z's shape and kind, row n = L(alpha_n) z[n] with L the lower Cholesky factor
    of the Toeplitz matrix of fgn_autocovariance(alpha_n, T).  Its cumulative sum is fractional Brownian motion with
    <x^2(k)> = k^alpha.  CUDA tensors go to the kernel (csrc/fbm.hip, one launch, equal exponents share a row of gamma;
    T <= ops.FGN_MAX_T, 1 <= C <= ops.FGN_MAX_C), anything else to the numpy restatement of the same recursion.  At
    alpha = 1 the result is z."""
    is_t = torch.is_tensor(z)
    if len(z.shape) != 3:
        raise ValueError(f"z must be [N, T, C], got {tuple(z.shape)}")
    N, T, C = (int(s) for s in z.shape)
    a = _alpha_vector(alphas, N)
    uniq, inv = torch.unique(a, return_inverse=True)
    if is_t and z.device.type == "cuda":
        from .. import ops
        if T > ops.FGN_MAX_T:
            raise ValueError(f"T = {T} steps on a GPU tensor, the kernel's limit is {ops.FGN_MAX_T} (ops.FGN_MAX_T)")
        if not 1 <= C <= ops.FGN_MAX_C:
            raise ValueError(f"z holds {C} axes, the kernel takes 1 .. {ops.FGN_MAX_C} (ops.FGN_MAX_C)")
        gamma = torch.from_numpy(fgn_autocovariance(uniq.numpy(), T)).to(z.device)
        return ops.fgn(z.detach().double().contiguous(), gamma, inv.to(z.device, torch.int32))
    zz = z.detach().double().numpy() if is_t else np.asarray(z, dtype=np.float64)
    out = _fgn_host(zz, fgn_autocovariance(uniq.numpy(), T)[inv.numpy()])
    return torch.from_numpy(out) if is_t else out


def _redrawn_normal(n, mean, var, lo, hi, generator, device):
    """n draws of N(mean, var), redrawn until inside [lo, hi] (64 rounds, then clamped), float32 on `device`."""
    x = mean + math.sqrt(var) * torch.randn(n, generator=generator, device=device)
    for _ in range(64):
        bad = (x < lo) | (x > hi)
        if not bool(bad.any()):
            break
        x = torch.where(bad, mean + math.sqrt(var) * torch.randn(n, generator=generator, device=device), x)
    return x.clamp(lo, hi)


def _draw_alphas(n, alphas, generator, gdev) -> torch.Tensor:
    """Per-particle exponents, float64 on the CPU: a number for all, a tensor / array of n values as given, or a (mean, var)
    pair (tuple or list) drawn N(mean, var) and redrawn until inside [ALPHA_MIN, ALPHA_MAX]; var = 0 draws nothing."""
    if isinstance(alphas, (tuple, list)):
        if len(alphas) != 2:
            raise ValueError("alphas must be a number, a (mean, var) pair, or a tensor / array with one exponent per particle")
        mean, var = float(alphas[0]), float(alphas[1])
        if var < 0 or not ALPHA_MIN <= mean <= ALPHA_MAX:
            raise ValueError(f"alphas = (mean {mean}, var {var}): the mean must lie in [{ALPHA_MIN}, {ALPHA_MAX}], var >= 0")
        if var > 0:
            return _redrawn_normal(n, mean, var, ALPHA_MIN, ALPHA_MAX, generator, gdev).to("cpu", torch.float64)
        alphas = mean
    return _alpha_vector(alphas, n)


def fbm_single_state(N: int, T: int, Ds=(1.0, 0.0), alphas=1.0, dt: float = 1.0,
                     generator: Optional[torch.Generator] = None, device="cpu"):
    """(T, N, 2) trajectories and (T, N, 3) labels [alpha, D, state=0] of fractional Brownian particles: stands in for
    ``andi_datasets.models_phenom().single_state(N, L=0, T, Ds=[mean, var], alphas=...)``.  alphas: a number, [N] values, or a
    (mean, var) pair drawn per particle (_draw_alphas).  Draws, in this order: D exactly as brownian_single_state draws it,
    the exponents of a pair with var > 0, torch.randn(T, N, 2).  Position 0 is 0 and the increments 1 .. T - 1 are
    fractional_gaussian_noise(z[1:]) * sqrt(2 D dt): per-axis increment variance 2 D dt, the law of disp_fbm
    (mitochondria_simulation/mitochnodria.py:436-476), and ensemble per-axis MSD 2 D dt k^alpha.  A scalar alphas = 1 gives
    brownian_single_state's trajectories bit for bit for the same seed.  device="cuda" runs csrc/fbm.hip."""
    mean, var = float(Ds[0]), float(Ds[1])
    D = torch.full((N,), mean, device=device)
    if var > 0:
        D = mean + math.sqrt(var) * torch.randn(N, generator=generator, device=device)
        for _ in range(64):                      # redraw non-positive coefficients (AnDi constrains D > 0)
            bad = D <= 1e-4
            if not bool(bad.any()):
                break
            D = torch.where(bad, mean + math.sqrt(var) * torch.randn(N, generator=generator, device=device), D)
        D = D.clamp_min(1e-4)
    alpha = _draw_alphas(N, alphas, generator, device)
    z = torch.randn(T, N, 2, generator=generator, device=device)
    steps = torch.empty_like(z)
    if T:
        steps[0] = 0.0
        noise = fractional_gaussian_noise(z[1:].double().permute(1, 0, 2).contiguous(), alpha)          # [N, T - 1, 2]
        steps[1:] = noise.permute(1, 0, 2).float() * torch.sqrt(2.0 * D * dt).view(1, N, 1)
    trajs = torch.cumsum(steps, dim=0)
    labels = torch.stack([alpha.to(z.device, torch.float32).view(1, N).expand(T, N), D.view(1, N).expand(T, N),
                          torch.zeros(T, N, device=device)], dim=-1)
    return trajs, labels


# ------------------------------------------------------------------------------------------------------------------------
# Multi-state diffusion: a Markov chain of states with one diffusion coefficient each (csrc/segment.hip)
# ------------------------------------------------------------------------------------------------------------------------
def _markov_host(u: np.ndarray, p0: np.ndarray, M: np.ndarray) -> np.ndarray:
    """The arithmetic of csrc/segment.hip::markov_kernel in numpy, vectorised over particles (include/mivit_hip.h,
    mivit_markov_states): u [N, T], p0 [K], M [K, K] float64 -> state [N, T] int32, bitwise the kernel's."""
    N, T = u.shape
    K = len(p0)
    rows = np.concatenate([p0.reshape(1, K), M.reshape(K, K)], axis=0)
    state = np.zeros((N, T), np.int32)
    row = np.zeros(N, np.int64)
    for t in range(T):
        pr = rows[row]                                                     # [N, K]
        c = pr[:, 0].copy()
        k = np.zeros(N, np.int64)
        open_ = ~(u[:, t] < c)                                             # still searching (a NaN searches to the end)
        for kk in range(1, K):
            k = np.where(open_, kk, k)
            c = np.where(open_, c + pr[:, kk], c)
            open_ = open_ & ~(u[:, t] < c)
        state[:, t] = k
        row = 1 + k
    return state


def _markov_args(Ds, M, p0):
    """(Ds [K], M [K, K], p0 [K]) as float64 arrays, checked; p0 = None is the stationary distribution of M."""
    from .. import ops
    Ds = np.asarray(torch.as_tensor(Ds).detach().cpu().numpy() if torch.is_tensor(Ds) else Ds, dtype=np.float64).reshape(-1)
    M = np.asarray(torch.as_tensor(M).detach().cpu().numpy() if torch.is_tensor(M) else M, dtype=np.float64)
    K = len(Ds)
    if not 1 <= K <= ops.MARKOV_MAX_K:
        raise ValueError(f"Ds holds {K} states, 1 .. {ops.MARKOV_MAX_K} (ops.MARKOV_MAX_K) are supported")
    if not (np.isfinite(Ds).all() and (Ds >= 0).all()):
        raise ValueError(f"Ds must be finite and >= 0, got {Ds.tolist()}")
    if M.shape != (K, K):
        raise ValueError(f"M must be [{K}, {K}], got {tuple(M.shape)}")
    if not ((M >= 0).all() and np.allclose(M.sum(axis=1), 1.0, rtol=0, atol=1e-9)):
        raise ValueError("every row of M must be a distribution: entries >= 0 that sum to 1")
    if p0 is None:
        # the left eigenvector of eigenvalue 1: (M^T - I) pi = 0 with sum(pi) = 1, by least squares
        A = np.concatenate([M.T - np.eye(K), np.ones((1, K))], axis=0)
        p0 = np.linalg.lstsq(A, np.concatenate([np.zeros(K), np.ones(1)]), rcond=None)[0]
        p0 = np.clip(p0, 0.0, None)
        p0 = p0 / p0.sum()
    else:
        p0 = np.asarray(torch.as_tensor(p0).detach().cpu().numpy() if torch.is_tensor(p0) else p0, dtype=np.float64).reshape(-1)
        if p0.shape != (K,) or not ((p0 >= 0).all() and abs(p0.sum() - 1.0) <= 1e-9):
            raise ValueError(f"p0 must be a distribution over the {K} states")
    return Ds, np.ascontiguousarray(M), np.ascontiguousarray(p0)


def markov_states(u, p0, M):
    """State paths of a Markov chain from uniform numbers: u [N, T] in [0, 1), p0 [K] the distribution of the first state, M
    [K, K] the transition matrix (row = from) -> state [N, T] int32 of u's kind.  state[n, 0] is the first k with u[n, 0] <
    p0[0] + .. + p0[k], state[n, t] the same on row M[state[n, t - 1]]; the last state catches rounding.  CUDA tensors go to
    the kernel (ops.markov_states, csrc/segment.hip), anything else to the numpy restatement, bitwise equal."""
    is_t = torch.is_tensor(u)
    if len(u.shape) != 2:
        raise ValueError(f"u must be [N, T], got {tuple(u.shape)}")
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else v                                  # noqa: E731
    p0h, Mh = np.asarray(host(p0), dtype=np.float64).reshape(-1), np.asarray(host(M), dtype=np.float64)
    _markov_args(np.zeros(len(p0h)), Mh, p0h)
    if is_t and u.device.type == "cuda":
        from .. import ops
        return ops.markov_states(u.detach().double().contiguous(), torch.from_numpy(p0h).to(u.device),
                                 torch.from_numpy(np.ascontiguousarray(Mh)).to(u.device))
    out = _markov_host(u.detach().double().numpy() if is_t else np.asarray(u, dtype=np.float64), p0h, Mh)
    return torch.from_numpy(out) if is_t else out


def _state_velocities(velocities, K: int, name: str):
    """velocities [K, 2] (vy, vx) per state as a float64 CPU tensor of finite numbers, or None where it is None or all zeros
    (the code path without it); ValueError otherwise."""
    if velocities is None:
        return None
    what = f"{name} must be real [{K}, 2] values (vy, vx), one pair per state"
    try:
        v = (velocities if torch.is_tensor(velocities) else torch.from_numpy(np.array(velocities))).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}, got {velocities!r}") from None
    if v.dtype == torch.bool or v.is_complex() or tuple(v.shape) != (K, 2):
        raise ValueError(f"{what}, got {v.dtype} {tuple(v.shape)}")
    v = v.double()
    if not bool(torch.isfinite(v).all()):
        raise ValueError(f"{name} must be finite")
    return v if bool((v != 0).any()) else None


def multi_state(N: int, T: int, Ds, M, p0=None, dt: float = 1.0, generator: Optional[torch.Generator] = None, device="cpu",
                return_states: bool = True, velocities=None):
    """(T, N, 2) Brownian trajectories whose diffusion coefficient follows a Markov chain, in the layout of
    brownian_single_state, and (with return_states) states [N, T] int64: stands in for
    ``andi_datasets.models_phenom().multi_state(N, L=0, T, Ds, M)`` with alpha = 1 in every state.  Ds [K] the coefficient of
    each state, M [K, K] the transition matrix per step, p0 [K] the distribution of the first state (default: the stationary
    distribution of M).  Draws, in this order: torch.rand(N, T) for the states, torch.randn(T, N, 2) for the steps.  Step t
    has variance 2 Ds[state[t]] dt per axis; position 0 is 0.  The state path comes from csrc/segment.hip on a GPU generator
    and from its numpy restatement otherwise.  velocities (default None: none): [K, 2] (vy, vx) per state in units of length
    per unit of dt (run-and-pause transport).  Step t adds velocities[state[t]] * dt, accumulated along the path in float64 and
    added to the trajectory once, rounded once; nothing is drawn for it, and None or all zeros give today's trajectories bit
    for bit.  What helpers/msd.segment_transport cuts."""
    Dsv, Mv, p0v = _markov_args(Ds, M, p0)
    Vv = _state_velocities(velocities, len(Dsv), "velocities")
    gdev = generator.device if generator is not None else torch.device(device)
    u = torch.rand(N, T, generator=generator, device=gdev, dtype=torch.float64)
    states = markov_states(u, p0v, Mv).long()
    scale = torch.sqrt(2.0 * torch.from_numpy(Dsv).to(gdev) * dt).float()[states]                            # [N, T]
    steps = torch.randn(T, N, 2, generator=generator, device=gdev) * scale.t().unsqueeze(-1)
    if T:
        steps[0] = 0.0
    trajs = torch.cumsum(steps, dim=0)
    if Vv is not None and T:
        inc = Vv.to(gdev)[states] * dt                                                                        # [N, T, 2] float64
        inc[:, 0] = 0.0
        trajs = (trajs.double() + torch.cumsum(inc, dim=1).transpose(0, 1)).float()                           # rounded once
    trajs = trajs.to(device)
    return (trajs, states.to(device)) if return_states else trajs


def psf_sigma_hr(props: dict) -> float:
    """Gaussian sigma on the upsampled grid (helpersGeneration.py: fwhm = wavelength / 2 * NA / psf_division_factor)."""
    fwhm = props["wavelength"] / 2 * props["NA"] / props.get("psf_division_factor", 1)
    return props["upsampling_factor"] / props["resolution"] * fwhm / 2.355


def render_frames(traj_px: torch.Tensor, nPosPerFrame: int, sigmas: Sequence[float], output_size: int,
                  upsampling_factor: int, spot_intensity: torch.Tensor, center: bool = False) -> torch.Tensor:
    """Noise-free frames.  traj_px: (N, T, 2) in pixels; sigmas: one hi-res sigma per PSF setting;
    spot_intensity: (N, F, p) amplitude of every sub-position.  Returns (N, len(sigmas), F, P, P)."""
    N, T, _ = traj_px.shape
    if T % nPosPerFrame != 0:
        raise Exception("T is not divisble by posPerFrame")
    if traj_px.device.type == "cuda":
        return _render_frames_hip(traj_px, nPosPerFrame, sigmas, output_size, upsampling_factor, spot_intensity, center)
    F_, p, P, up = T // nPosPerFrame, nPosPerFrame, output_size, upsampling_factor
    G = P * up
    dev = traj_px.device
    seg = traj_px.reshape(N, F_, p, 2)
    if center:
        seg = seg - seg.mean(dim=2, keepdim=True)
    seg = seg * up
    limit = (G - 1) // 2                                   # same (integer) limit as the reference grid
    axis = torch.linspace(-limit, limit, G, device=dev, dtype=traj_px.dtype)
    out = []
    for s in sigmas:
        # spot / spot_max per axis, as ONE exponential of the difference of squared distances: the reference divides two
        # float64 Gaussians (a spot that left the frame still peaks at full intensity on the border); fp32 factors would
        # underflow to 0 / 0 there.  The difference is taken as (d - dpk) (d + dpk), dpk the distance to the nearest grid
        # point: for a spot hundreds of grid steps outside the frame the two squares are near 1e5 and their fp32 roundings
        # do not cancel (2e-5 in the argument under a PSF of 3 pixels), while d - dpk is a difference of grid points
        prof, profy = (_peak_normalised_profile(axis.view(1, 1, 1, G) - seg[..., k:k + 1], s) for k in (0, 1))   # (N,F,p,G)
        px = prof.reshape(N, F_, p, P, up).mean(dim=-1)                   # mean pooling of each 1-D profile
        py = profy.reshape(N, F_, p, P, up).mean(dim=-1)
        # frame[y, x] = sum_p a_p * py_p[y] * px_p[x]
        out.append(torch.einsum("nfp,nfpy,nfpx->nfyx", spot_intensity, py, px))
    return torch.stack(out, dim=1)


def _peak_normalised_profile(d, s):
    """exp(-(d^2 - min d^2) / 2 s^2) along the last axis"""
    dpk = torch.gather(d, -1, d.abs().argmin(dim=-1, keepdim=True))
    return torch.exp(-((d - dpk) * (d + dpk)) / (2 * s * s))


def _render_frames_hip(traj_px, nPosPerFrame, sigmas, output_size, upsampling_factor, spot_intensity, center):
    """GPU tensors: the hand-written kernel (csrc/render.hip, mivit_render_frames) -- one workgroup per (sequence, frame, PSF)."""
    import ctypes
    from .. import _native as Nat
    N, T, _ = traj_px.shape
    F_ = T // nPosPerFrame
    dev = traj_px.device
    traj = traj_px.contiguous().float()
    amp = spot_intensity.to(dev).expand(N, F_, nPosPerFrame).contiguous().float()
    sig = torch.tensor([float(s) for s in sigmas], dtype=torch.float32, device=dev)
    out = torch.empty(N, len(sig), F_, output_size, output_size, dtype=torch.float32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for n0 in range(0, N, 65535):                     # grid.y limit
        n1 = min(N, n0 + 65535)
        Nat.check(Nat.lib.mivit_render_frames(vp(traj[n0:n1]), n1 - n0, T, nPosPerFrame, vp(sig), len(sig), output_size,
                                              upsampling_factor, vp(amp[n0:n1]), int(bool(center)), vp(out[n0:n1]),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mivit_render_frames")
    return out.to(traj_px.dtype)


def clipped_background(shape, mean: float, std: float, generator=None, device="cpu"):
    """np.clip(np.random.normal(mean, std), 0, mean + 3 std)  (helpersGeneration.py:312-313)."""
    if std <= 0:
        return torch.full(shape, float(min(max(mean, 0.0), mean)), device=device)
    return (mean + std * torch.randn(shape, generator=generator, device=device)).clamp(0.0, mean + 3 * std)


def trajectories_to_video(trajectories, nPosPerFrame: int, center: bool = False, image_props: Optional[dict] = None,
                          generator: Optional[torch.Generator] = None, device=None) -> torch.Tensor:
    """(N, T, 2) trajectories -> (N, T / nPosPerFrame, P, P) float32 videos (helpersGeneration.py:128-319).
    The y axis is flipped like the reference does, without mutating the caller's array."""
    props = dict(DEFAULT_IMAGE_PROPS)
    props.update(image_props or {})
    traj = _as_tensor(trajectories, device).clone()
    dev = traj.device
    traj[:, :, 1] *= -1
    if props["trajectory_unit"] != -1:
        traj = traj * props["trajectory_unit"] / (props["resolution"] * 1e9)
    N, T, _ = traj.shape
    if T % nPosPerFrame != 0:
        raise Exception("T is not divisble by posPerFrame")
    F_ = T // nPosPerFrame
    pm, ps = props["particle_intensity"]
    bm, bs = props["background_intensity"]
    if pm > 1e-4 and ps > 1e-4:
        amp = pm / nPosPerFrame + (ps / nPosPerFrame) * torch.randn(N, F_, nPosPerFrame, generator=generator, device=dev)
    else:
        amp = torch.zeros(N, F_, nPosPerFrame, device=dev)
    vid = render_frames(traj, nPosPerFrame, [psf_sigma_hr(props)], props["output_size"], props["upsampling_factor"],
                        amp, center)[:, 0]
    vid = vid + clipped_background(vid.shape, bm, bs, generator, dev)
    pn = props["poisson_noise"]
    if pn != -1:
        vid = vid * torch.poisson(torch.full(vid.shape, float(pn), device=dev), generator=generator) / pn
    return vid.float()


def normalize_images(images, background_mean=None, background_sigma=None, theoretical_max=None, clip_image=False):
    """(im - (bg_mean - bg_sigma)) / (theoretical_max - (bg_mean - bg_sigma))  (helpersGeneration.py:356-400)."""
    images = _as_tensor(images, None)
    if background_mean is None:
        background_mean = float(images.mean())
    if background_sigma is None:
        background_sigma = float(images.std(unbiased=False))
    if theoretical_max is None:
        theoretical_max = float(images.max())
    denom = theoretical_max - (background_mean - background_sigma)
    if denom == 0:
        raise ValueError("Denominator in normalization is zero. Check your inputs.")
    out = (images - (background_mean - background_sigma)) / denom
    if clip_image:
        out = out.clamp(0, 1.5)
    return out, (background_mean, background_sigma, theoretical_max)


# ------------------------------------------------------------------------------------------------------------------------
# Denoising experiment: multi-setting videos, Gaussian filter, RL-TV deconvolution (helpersGeneration.py:422-660)
# ------------------------------------------------------------------------------------------------------------------------

def create_gaussian_psf(size=9, sigma=1.3):
    """Normalised Gaussian PSF of odd side (an even size grows by one), float64 (helpersGeneration.py:591-600)."""
    if size % 2 == 0:
        size += 1
    ax = np.arange(-(size // 2), size // 2 + 1)
    x, y = np.meshgrid(ax, ax)
    psf = np.exp(-(x ** 2 + y ** 2) / (2 * sigma ** 2))
    psf /= psf.sum()
    return psf


def tv_gradient(image):
    """Gradient of the total variation over the last two axes (helpersGeneration.py:542-555), in image's dtype: forward
    differences with the last column / row repeated, normalised by sqrt(dx^2 + dy^2 + 1e-8)."""
    image = np.asarray(image)
    dt = image.dtype.type
    dx = np.zeros_like(image)
    dy = np.zeros_like(image)
    dx[..., :, :-1] = image[..., :, 1:] - image[..., :, :-1]
    dy[..., :-1, :] = image[..., 1:, :] - image[..., :-1, :]
    mag = np.sqrt((dx * dx + dy * dy) + dt(1e-8))
    dxn, dyn = dx / mag, dy / mag
    grad = np.zeros_like(image)
    grad[..., :, :-1] -= dxn[..., :, :-1]
    grad[..., :, 1:] += dxn[..., :, :-1]
    grad[..., :-1, :] -= dyn[..., :-1, :]
    grad[..., 1:, :] += dyn[..., :-1, :]
    return grad


def _conv_same(x, k):
    """scipy.signal.fftconvolve(x, k, mode='same') over the last two axes as a zero-padded direct sum in float64, taps in
    row-major (a, b) order from 0.0, one multiply and one add each -- the order of csrc/deconv.hip."""
    K = k.shape[0]
    H, W = x.shape[-2:]
    halo = K - 1 - (K - 1) // 2
    xp = np.zeros(x.shape[:-2] + (H + K - 1, W + K - 1), np.float64)
    xp[..., halo:halo + H, halo:halo + W] = x
    acc = np.zeros(x.shape, np.float64)
    for a in range(K):
        for b in range(K):
            acc += k[a, b] * xp[..., K - 1 - a:K - 1 - a + H, K - 1 - b:K - 1 - b + W]
    return acc


def _check_iterations(iterations_list):
    its = [int(i) for i in iterations_list]
    if not its or its[0] < 0 or any(b <= a for a, b in zip(its, its[1:])):
        raise ValueError(f"iterations_list must be non-empty, non-negative and strictly increasing, got {list(iterations_list)}")
    return its


def _rl_tv_frames(frames, psf, iterations_list, tv_weight):
    """Host RL-TV of a stack of frames [..., H, W] -> [len(iterations_list), ..., H, W] float32: the estimate after every
    listed (0-based) iteration.  Same precision per step as richardson_lucy_tv_iter_list (helpersGeneration.py:571-589):
    fp64 convolutions and division, fp32 estimate and TV gradient."""
    its = _check_iterations(iterations_list)
    psf = np.asarray(psf, np.float64)
    if psf.ndim != 2 or psf.shape[0] != psf.shape[1]:
        raise ValueError(f"psf must be square [K, K], got {psf.shape}")
    image = np.clip(np.asarray(frames, np.float32), np.float32(1e-6), None).astype(np.float64)
    mirror = psf[::-1, ::-1]
    tvw = np.float32(tv_weight)
    est = np.full(image.shape, 0.5, np.float32)
    out = np.empty((len(its),) + image.shape, np.float32)
    for i in range(its[-1] + 1):
        rel = image / (_conv_same(est, psf) + 1e-6)
        est = (est.astype(np.float64) * _conv_same(rel, mirror)).astype(np.float32)
        est = np.clip(est - tvw * tv_gradient(est), np.float32(0), np.float32(1))
        if i in its:
            out[its.index(i)] = est
    return out


def richardson_lucy_tv(image, psf, iterations=20, tv_weight=0.01):
    """RL-TV estimate after `iterations` iterations, float32 (helpersGeneration.py:557-568)."""
    image = np.asarray(image)
    if iterations <= 0:
        return np.full(image.shape, 0.5, np.float32)
    return _rl_tv_frames(image, psf, [iterations - 1], tv_weight)[0]


def richardson_lucy_tv_iter_list(image, psf, iterations_list, out_array, tv_weight=0.01):
    """RL-TV with a snapshot after each listed 0-based iteration written to out_array[k]; returns the final estimate
    (helpersGeneration.py:571-589).  Unlike the reference the list must be strictly increasing (ValueError otherwise:
    the reference leaves slots of out_array unwritten)."""
    snaps = _rl_tv_frames(image, psf, iterations_list, tv_weight)
    for k in range(len(snaps)):
        out_array[k] = snaps[k]
    return snaps[-1]


def _rl_tv_batch(tensor, psf, iterations_list, tv_weight):
    """[B, S, H, W] -> [B, len(iterations_list), S, H, W]: the kernel for GPU tensors, the host restatement otherwise."""
    its = _check_iterations(iterations_list)
    if isinstance(tensor, torch.Tensor) and tensor.device.type == "cuda":
        from .. import ops
        return ops.rl_tv_deconvolve(tensor.float(), psf, its, tv_weight)
    arr = tensor.detach().cpu().numpy() if isinstance(tensor, torch.Tensor) else np.asarray(tensor)
    return np.moveaxis(_rl_tv_frames(arr, psf, its, tv_weight), 0, 1)


def apply_rl_tv_tensor(tensor, psf, n_iters=10, tv_weight=0.01):
    """richardson_lucy_tv of every 9x9 frame of a [B, seq, 9, 9] tensor, same dtype and device
    (helpersGeneration.py:603-613)."""
    B, seq, H, W = tensor.shape
    assert H == 9 and W == 9, "Only images of shape 9x9 are supported"
    if n_iters <= 0:
        return torch.full(tuple(tensor.shape), 0.5, dtype=tensor.dtype, device=tensor.device)
    out = _rl_tv_batch(tensor, psf, [n_iters - 1], tv_weight)[:, 0]
    return torch.as_tensor(out).to(dtype=tensor.dtype, device=tensor.device)


def apply_rl_tv_tensor_iter_list(tensor, psf, iterations_list=[2, 5, 10], tv_weight=0.01):
    """[B, seq, 9, 9] -> [B, len(iterations_list), seq, 9, 9]: RL-TV snapshots of every frame (helpersGeneration.py:616-632).
    numpy / CPU input gives numpy in the input's dtype, as the reference; a GPU tensor gives a GPU float32 tensor (the
    reference always returns numpy).  The list must be strictly increasing."""
    B, seq, H, W = tensor.shape
    assert H == 9 and W == 9, "Only images of shape 9x9 are supported"
    out = _rl_tv_batch(tensor, psf, iterations_list, tv_weight)
    if isinstance(out, torch.Tensor):
        return out
    dtype = tensor.detach().cpu().numpy().dtype if isinstance(tensor, torch.Tensor) else np.asarray(tensor).dtype
    return out.astype(dtype, copy=False)


def _gaussian_weights(sigma, truncate):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, int(truncate * sigma + 0.5)): w[0] centre .. w[r]."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[r:]


def gaussian_filter_frames(frames, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter(frame, sigma, mode='nearest', truncate) of every [H, W] frame, float32 out: what
    ski.filters.gaussian(frame, sigma) does for a float frame (helpersGeneration.py:530).  GPU tensors go to
    csrc/deconv.hip; anything else to the same separable fp64 passes in numpy (axis 0, then axis 1, replicated borders,
    symmetric taps summed from the outermost in as scipy's correlate1d does)."""
    if isinstance(frames, torch.Tensor) and frames.device.type == "cuda":
        from .. import ops
        return ops.gaussian_filter_frames(frames.float(), sigma, truncate)
    is_t = isinstance(frames, torch.Tensor)
    x = (frames.detach().cpu().numpy() if is_t else np.asarray(frames)).astype(np.float64)
    w = _gaussian_weights(sigma, truncate)
    for axis in (-2, -1):
        n = x.shape[axis]
        idx = np.arange(n)
        acc = x * w[0]
        for k in range(len(w) - 1, 0, -1):
            lo = np.take(x, np.clip(idx - k, 0, n - 1), axis=axis)
            hi = np.take(x, np.clip(idx + k, 0, n - 1), axis=axis)
            acc = acc + (lo + hi) * w[k]
        x = acc
    out = x.astype(np.float32)
    return torch.from_numpy(out) if is_t else out


def _normal(shape, mean, std, generator, device):
    """mean + std * N(0, 1), drawn on the generator's device and moved to `device`."""
    gdev = generator.device if generator is not None else device
    return (mean + std * torch.randn(shape, generator=generator, device=gdev)).to(device)


def _poisson(rate, generator):
    gdev = generator.device if generator is not None else rate.device
    return torch.poisson(rate.to(gdev), generator=generator).to(rate.device)


def trajectories_to_video_multiple_settings(trajectories, nPosPerFrame, center=False, image_props={}, generator=None,
                                            device=None):
    """(N, T, 2) trajectories -> four (N, T / nPosPerFrame, P, P) float32 videos of the same frames
    (helpersGeneration.py:422-536): no noise, + clipped Gaussian background, Poisson(frame * pn) / pn of that, and
    gaussian_filter(Poisson frame, sigma=0.5).  One particle intensity ~ N(mean, std) per frame, shared by its
    sub-positions (:506-513).  This function's own defaults apply (poisson_noise 1, :440-456).  The y axis is flipped as
    the reference does, without mutating the caller's array."""
    props = dict(DEFAULT_IMAGE_PROPS)
    props["poisson_noise"] = 1
    props.update(image_props or {})
    traj = _as_tensor(trajectories, device).clone()
    dev = traj.device
    traj[:, :, 1] *= -1
    N, T, _ = traj.shape
    if T % nPosPerFrame != 0:
        raise Exception("T is not divisble by posPerFrame")
    if props["trajectory_unit"] != -1:
        traj = traj * props["trajectory_unit"] * 1e-9 / props["resolution"]
    F_ = T // nPosPerFrame
    pm, ps = props["particle_intensity"]
    bm, bs = props["background_intensity"]
    frame_int = _normal((N, F_, 1), pm, ps, generator, dev)
    if pm > 1e-4 and ps > 1e-4:
        amp = (frame_int / nPosPerFrame).expand(N, F_, nPosPerFrame)
    else:
        amp = torch.zeros(N, F_, nPosPerFrame, device=dev)
    clean = render_frames(traj, nPosPerFrame, [psf_sigma_hr(props)], props["output_size"], props["upsampling_factor"],
                          amp, center)[:, 0].float()
    bg = _normal(clean.shape, bm, bs, generator, dev).clamp(0.0, bm + 3 * bs) if bs > 0 else \
        torch.full(clean.shape, float(max(bm, 0.0)), device=dev)
    noisy = clean + bg
    pn = props["poisson_noise"]
    poisson = _poisson(noisy * pn, generator) / pn
    filtered = gaussian_filter_frames(poisson, 0.5)
    return clean, noisy, poisson, torch.as_tensor(filtered).to(dev)


def trajs_to_vid_norm_rl(trajectories, nPosPerFrame, center, image_props, rl_iterations, poisson_index=2, generator=None,
                         device=None):
    """(N, T, 2) -> (N, 4 + len(rl_iterations), F, P, P) float32 (helpersGeneration.py:635-660): the four settings of
    trajectories_to_video_multiple_settings normalised by normalize_images(bg_mean, bg_sigma, part_mean + bg_mean), then
    RL-TV snapshots (create_gaussian_psf(sigma=1)) of channel `poisson_index`.  numpy input gives numpy (the reference);
    a GPU tensor (or device="cuda") keeps everything on the GPU and gives a GPU tensor."""
    bg_mean, bg_sigma = image_props["background_intensity"]
    part_mean = image_props["particle_intensity"][0]
    psf = create_gaussian_psf(sigma=1)
    videos = torch.stack(trajectories_to_video_multiple_settings(trajectories, nPosPerFrame, center=center,
                                                                 image_props=image_props, generator=generator,
                                                                 device=device), dim=1)
    videos, _ = normalize_images(videos, bg_mean, bg_sigma, part_mean + bg_mean)
    videos = videos.float()
    rl = apply_rl_tv_tensor_iter_list(videos[:, poisson_index], psf, rl_iterations)
    out = torch.cat([videos, torch.as_tensor(rl).to(videos.device)], dim=1)
    return out if out.device.type == "cuda" else out.numpy()


# ------------------------------------------------------------------------------------------------------------------------
# Whole fields of view: many particles in one [F, H, W] movie, with the truth table (csrc/movie.hip)
# ------------------------------------------------------------------------------------------------------------------------
MOVIE_MAX_RADIUS = 64        # limits of csrc/movie.hip (ops.MOVIE_MAX_RADIUS, ops.MOVIE_MAX_NPOS, ops.MOVIE_MAX_UP)
MOVIE_MAX_NPOS = 256
MOVIE_MAX_UP = 64
_MOVIE_MAX_COORD = 2.0 ** 30


def default_movie_radius(sigma_hr: float, upsampling_factor: int) -> int:
    """ceil(5 sigma_hr / up) + 1 camera pixels: beyond it a spot is below exp(-12.5) = 4e-6 of its peak."""
    return int(math.ceil(5.0 * float(sigma_hr) / int(upsampling_factor))) + 1


def _check_movie_args(pos_shape, amp_shape, sigma_hr, H, W, up, radius, first, last):
    if len(amp_shape) != 3:
        raise ValueError(f"amp must be [Np, F, nPosPerFrame], got {tuple(amp_shape)}")
    Np, F_, npos = (int(v) for v in amp_shape)
    if len(pos_shape) != 3 or pos_shape[2] != 2 or pos_shape[0] != Np:
        raise ValueError(f"pos_yx must be [{Np}, T, 2], got {tuple(pos_shape)}")
    if npos < 1 or pos_shape[1] % npos != 0:
        raise ValueError("T is not divisble by posPerFrame")
    if pos_shape[1] // npos != F_ or F_ < 1:
        raise ValueError(f"pos_yx holds {pos_shape[1] // npos} frames of {npos} sub-positions, amp {F_}; at least one is needed")
    if npos > MOVIE_MAX_NPOS:
        raise ValueError(f"nPosPerFrame = {npos}, the limit is {MOVIE_MAX_NPOS} (MOVIE_MAX_NPOS)")
    if int(up) != up or not 1 <= up <= MOVIE_MAX_UP:
        raise ValueError(f"upsampling_factor must be an integer from 1 to {MOVIE_MAX_UP}, got {up}")
    if int(H) != H or int(W) != W or not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
        raise ValueError(f"H and W must be integers from 1 to 2^24, got {H}, {W}")
    s = float(sigma_hr)
    if not (s > 0 and math.isfinite(s) and 0 < np.float32(1) / (np.float32(2) * np.float32(s) * np.float32(s)) < np.inf):
        raise ValueError(f"sigma_hr = {sigma_hr} is not a usable width")
    if radius is None:
        radius = default_movie_radius(s, up)
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= radius <= MOVIE_MAX_RADIUS:
        raise ValueError(f"radius must be an integer from 0 to {MOVIE_MAX_RADIUS} (MOVIE_MAX_RADIUS), got {radius}")
    if (first is None) != (last is None):
        raise ValueError("first and last must both be given or both be None")
    if first is not None:
        fi, la = torch.as_tensor(first), torch.as_tensor(last)
        if fi.shape != (Np,) or la.shape != (Np,) or fi.is_floating_point() or la.is_floating_point():
            raise ValueError(f"first and last must be integer [{Np}]")
        if bool((fi > la).any()):
            raise ValueError("first > last")
    return Np, F_, npos, int(up), int(radius)


def _movie_profile(idx, c, up, sigma_hr):
    """prof(i; c) of csrc/movie.hip in float64 for camera pixels idx [..., n] and positions c [..., 1]."""
    u = c * up + (up - 1) / 2.0
    dpk = torch.round(u) - u                                   # round-half-to-even = rint
    g = idx.unsqueeze(-1) * up + torch.arange(up, dtype=torch.float64, device=c.device)      # [..., n, up]
    d = g - u.unsqueeze(-1)
    return torch.exp(-(d * d - (dpk * dpk).unsqueeze(-1)) / (2.0 * sigma_hr * sigma_hr)).mean(dim=-1)


def render_movie(pos_yx, amp, sigma_hr: float, H: int, W: int, upsampling_factor: int, radius: Optional[int] = None,
                 first=None, last=None) -> torch.Tensor:
    """Noise-free movie [F, H, W] of Np particles in one field of view.  pos_yx [Np, F * p, 2]: positions (y, x) = (row,
    column) in camera pixels, pixel centres at integers (the convention of the tracking tables; no flip, no unit conversion),
    p sub-positions per frame; amp [Np, F, p]: the intensity of every sub-position; first / last [Np] integers (optional):
    particle n is rendered in the frames first[n] .. last[n] inclusive.

    The image model is one spot of the reference (helpersGeneration.py:283-310) -- a Gaussian of sigma_hr on the
    upsampling_factor-times finer grid, rescaled to its PEAK on that grid, mean-pooled -- summed over sub-positions and
    particles: fine sample g = i up + k of pixel i sits at g, a position c at u = c up + (up - 1) / 2, g* = rint(u),
    dpk = g* - u, prof(i; c) = mean_k exp(-((g - u)^2 - dpk^2) / (2 sigma_hr^2)), and a sub-position adds
    amp prof(y; c_y) prof(x; c_x) to the pixels with |y - rint(c_y)| <= radius and |x - rint(c_x)| <= radius, nothing
    elsewhere (default radius ceil(5 sigma_hr / up) + 1; at most MOVIE_MAX_RADIUS).  For odd P up this is
    render_frames(center=False) on a P x P field with c = c_ref + (P - 1) / 2 and x / y swapped, except that the peak is taken
    on the unbounded grid: a particle that leaves the field fades out instead of being rescaled onto the border.  A
    sub-position whose position or amplitude is not finite (or |coordinate| >= 2^30) contributes nothing.

    CUDA tensors go to the kernel (csrc/movie.hip, mivit_render_movie; float32 in and out).  Anything else (CPU tensors, numpy)
    goes to a vectorised float64 restatement of the same definition, truncation included, and returns a float64 CPU tensor:
    the kernel's yardstick."""
    is_cuda = torch.is_tensor(pos_yx) and pos_yx.device.type == "cuda"
    pos = pos_yx if torch.is_tensor(pos_yx) else torch.as_tensor(np.asarray(pos_yx))
    am = amp if torch.is_tensor(amp) else torch.as_tensor(np.asarray(amp))
    Np, F_, npos, up, radius = _check_movie_args(pos.shape, am.shape, sigma_hr, H, W, upsampling_factor, radius, first, last)
    H, W = int(H), int(W)
    if is_cuda:
        from .. import ops
        dev = pos.device
        fi = la = None
        if first is not None:
            fi = torch.as_tensor(first).to(dev, torch.int32).contiguous()
            la = torch.as_tensor(last).to(dev, torch.int32).contiguous()
        return ops.render_movie(pos.float().contiguous(), am.to(dev).float().contiguous(), float(sigma_hr), up, radius, H, W,
                                fi, la)
    pos = pos.detach().to("cpu", torch.float64).reshape(Np, F_, npos, 2)
    am = am.detach().to("cpu", torch.float64)
    sigma = float(sigma_hr)
    ok = torch.isfinite(pos).all(dim=-1) & (pos.abs() < _MOVIE_MAX_COORD).all(dim=-1) & torch.isfinite(am)
    if first is not None:
        fr = torch.arange(F_).view(1, F_, 1)
        ok &= (torch.as_tensor(first).long().view(Np, 1, 1) <= fr) & (fr <= torch.as_tensor(last).long().view(Np, 1, 1))
    movie = torch.zeros(F_ * H * W, dtype=torch.float64)
    off = torch.arange(-radius, radius + 1, dtype=torch.float64)
    frame_base = (torch.arange(F_) * (H * W)).view(F_, 1, 1, 1)
    for n in range(Np):                                       # particles ascending; one scatter-add per particle
        c = torch.where(ok[n].unsqueeze(-1), pos[n], torch.zeros((), dtype=torch.float64))      # [F, p, 2]
        centre = torch.round(c)
        rows, cols = centre[..., 0:1] + off, centre[..., 1:2] + off                              # [F, p, 2 r + 1]
        py = _movie_profile(rows, c[..., 0:1], up, sigma) * torch.where(ok[n], am[n], torch.zeros((), dtype=torch.float64)).unsqueeze(-1)
        px = _movie_profile(cols, c[..., 1:2], up, sigma)
        inside = ((rows >= 0) & (rows < H)).unsqueeze(-1) & ((cols >= 0) & (cols < W)).unsqueeze(-2) & ok[n].view(F_, npos, 1, 1)
        val = py.unsqueeze(-1) * px.unsqueeze(-2)                                               # [F, p, 2 r + 1, 2 r + 1]
        idx = frame_base + rows.long().clamp(0, H - 1).unsqueeze(-1) * W + cols.long().clamp(0, W - 1).unsqueeze(-2)
        movie.index_add_(0, idx[inside], val[inside])
    return movie.view(F_, H, W)


def _draw_diffusion_coefficients(n, Ds, generator, gdev):
    """Per-particle D: a tensor / array of n values as given, a number for all, or a (mean, var) pair drawn as
    brownian_single_state draws it (N(mean, var), redrawn until positive)."""
    if torch.is_tensor(Ds) or isinstance(Ds, np.ndarray):
        D = torch.as_tensor(Ds).detach().to("cpu", torch.float64).reshape(-1)
        if D.numel() != n:
            raise ValueError(f"Ds must hold one coefficient per particle ({n}), got {D.numel()}")
    elif isinstance(Ds, (int, float)):
        D = torch.full((n,), float(Ds), dtype=torch.float64)
    elif len(Ds) == 2:
        mean, var = float(Ds[0]), float(Ds[1])
        D = torch.full((n,), mean, device=gdev)
        if var > 0:
            D = mean + math.sqrt(var) * torch.randn(n, generator=generator, device=gdev)
            for _ in range(64):
                bad = D <= 1e-4
                if not bool(bad.any()):
                    break
                D = torch.where(bad, mean + math.sqrt(var) * torch.randn(n, generator=generator, device=gdev), D)
            D = D.clamp_min(1e-4)
        D = D.to("cpu", torch.float64)
    else:
        raise ValueError("Ds must be a (mean, var) pair, a number, or a tensor / array with one coefficient per particle")
    if not bool(torch.isfinite(D).all()) or bool((D < 0).any()):
        raise ValueError("diffusion coefficients must be finite and >= 0")
    return D


def _movie_geometries(geometry, geometry_of, boundary, Np, H, W, margin):
    """simulate_movie's filaments: (the packed geometries with the vertices flipped to (row, col) = (y, x), geometry id [Np]
    int64).  ValueError for a vertex outside the margin, a geometry_of outside [0, G) and an unknown boundary."""
    from . import geometry as _geometry
    if boundary not in _geometry.BOUNDARIES:
        raise ValueError(f"boundary must be one of {_geometry.BOUNDARIES}, got {boundary!r}")
    geoms = [geometry] if isinstance(geometry, _geometry.Geometry) else list(geometry)
    packed = _geometry.pack_geometries(geoms)
    G = len(geoms)
    for g in range(G):
        for v in range(packed["vert_offsets"][g], packed["vert_offsets"][g + 1]):
            x, y = packed["verts"][v]
            if not (margin <= x <= W - 1 - margin and margin <= y <= H - 1 - margin):
                raise ValueError(f"geometry {g}: vertex {v - packed['vert_offsets'][g]} at (x, y) = ({x}, {y}) lies outside "
                                 f"[{margin}, {W - 1 - margin}] x [{margin}, {H - 1 - margin}]")
    if geometry_of is None:
        geom_id = np.arange(Np, dtype=np.int64) % G
    else:
        gof = torch.as_tensor(geometry_of).detach().cpu()
        if gof.is_floating_point() or gof.dtype == torch.bool or tuple(gof.shape) != (Np,):
            raise ValueError(f"geometry_of must be integer [{Np}], got {gof.dtype} {tuple(gof.shape)}")
        geom_id = gof.long().numpy()
        if Np and (geom_id.min() < 0 or geom_id.max() >= G):
            raise ValueError(f"geometry_of must lie in [0, {G})")
    packed["verts"] = np.ascontiguousarray(packed["verts"][:, ::-1])
    return packed, geom_id


def simulate_movie(n_particles: int, n_frames: int, H: int, W: int, Ds, nPosPerFrame: int, image_props: Optional[dict] = None,
                   margin: Optional[float] = None, lifetimes=None, generator: Optional[torch.Generator] = None, device="cpu",
                   blink=None, alphas=None, geometry=None, geometry_of=None, boundary="clamp", states=None, drift=None, camera=None,
                   confinement=None, velocity=None):
    """A field of view with known truth -> (movie [F, H, W] float32 on `device`, truth).

    n_particles free Brownian particles: start positions uniform in [margin, H - 1 - margin] x [margin, W - 1 - margin]
    (default margin: the rendering radius, so every spot starts inside), nPosPerFrame sub-positions per frame with steps
    N(0, 2 D / nPosPerFrame) per axis, D per particle in pixels^2 per frame (Ds: see _draw_diffusion_coefficients).  lifetimes
    [Np, 2] integers (first, last): the frames 0 <= first <= last < n_frames in which a particle is visible (default: all).
    Image: render_movie with the PSF of image_props (psf_sigma_hr, upsampling_factor), then, in the order and with the helpers
    of trajectories_to_video, amplitudes particle_intensity / nPosPerFrame per sub-position (zero unless mean and std exceed
    1e-4, as there), + clipped_background, * Poisson(poisson_noise) / poisson_noise; poisson_noise = -1 and a zero background
    std give a noise-free movie.  output_size, resolution's unit conversion and the y flip of trajectories_to_video do not
    apply: positions are pixel indices (y, x).  A generator must live on `device`; the same seed gives the same movie on the
    same device.

    truth: dict of tensors on `device`: frame (int64), y, x (float64: the mean of the frame's sub-positions), particle_id
    (int64), one row per visible particle-frame sorted by particle and then by frame; offsets [Np + 1] int64, CSR over those
    rows (the layout of tracking.tracks_table_by_track: msd.track_msd(stack([y, x], 1), offsets) runs on it as it is); D [Np]
    float64; pos [Np, F * nPosPerFrame, 2] float32 and amp [Np, F, nPosPerFrame] float32, what was rendered; first, last [Np]
    int64.

    blink (default None: no dark frames, the code path without it): a float in [0, 1), the probability that a particle is dark
    in a frame of its lifetime, drawn from `generator` after the amplitudes and before rendering; or a bool [Np, F] mask, True
    = dark.  A dark particle-frame has all its sub-position amplitudes set to zero.  truth keeps one row per frame of the
    lifetime (offsets is unchanged) and gains visible (bool per row, False on a dark frame); truth["amp"] is the zeroed one.
    tracking.score_tracking therefore counts a dark frame as a truth row: a filled row of a gap-closed track that lands on it
    is a match, an unfilled gap a miss.

    alphas (default None: Brownian motion, the code path without it): the anomalous exponent per particle, a number, [Np]
    values or a (mean, var) pair (_draw_alphas; a pair is drawn from `generator` right after D).  The sub-position steps are
    then fractional_gaussian_noise(z) * sqrt(2 D / nPosPerFrame^alpha) with z = randn(Np, T, 2) drawn where the Brownian steps
    are, so the MSD per axis after k frames is 2 D k^alpha; on a GPU generator T = F * nPosPerFrame <= ops.FGN_MAX_T.  truth
    gains alpha [Np] float64.  alphas = ones gives the movie and truth of alphas = None bit for bit.

    geometry (default None: free motion in the plane, the code path without it): a helpers/geometry.Geometry or a sequence of
    G of them, filaments the particles are confined to; geometry_of [Np] integers names each particle's (default
    arange(Np) % G); boundary "clamp" (the reference's Geometry.map_displacements) or "reflect" is what happens at a filament's
    two ends.  Vertices are (x, y) and must lie in [margin, W - 1 - margin] x [margin, H - 1 - margin].  In place of the start
    positions one torch.rand(Np) is drawn, times the filament's total length the start arc; then z = randn(Np, T, 1), and
    the steps z * sqrt(2 D / nPosPerFrame) (with alphas: the fractional noise as above, one axis) go through
    geometry.map_displacements (csrc/confine.hip on a GPU generator).  D is the 1-D coefficient ALONG the filament:
    <ds^2> = 2 D k^alpha after k frames.  truth gains arc [Np, T] float64, edge [Np, T] int32 (within the particle's geometry)
    and geometry_id [Np] int64; truth["pos"] is the mapped position in float32.  truth["y"] and truth["x"] remain the means of
    a frame's sub-positions: where a frame's sub-positions go round a corner the mean lies off the filament.

    states (default None: one D per particle, the code path without it): a dict {"Ds": [K], "M": [K, K], "p0": optional [K],
    "path": optional} of a multi-state particle (multi_state, _markov_args); the argument Ds must then be None.  u = rand(Np,
    F) is drawn where D is drawn otherwise and markov_states(u, p0, M) is the state of every particle in every frame (csrc/
    segment.hip on a GPU generator); "path", integer [Np, F] in [0, K), plants the states instead and nothing is drawn for
    them.  The state is constant over the sub-positions of a frame: sub-step t of frame f has variance 2 Ds[state[p, f]] /
    nPosPerFrame.  truth gains state (int64 per row) and D_row (float64 per row); truth["D"] is the mean of D_row over the
    lifetime, so score_tracking keeps working.  Not together with alphas; with a geometry the steps run along the filament.
    "velocity", [K, 2] (vy, vx) per state in pixels per frame (run-and-pause transport): sub-step t of frame f adds
    velocity[state[p, f]] / nPosPerFrame, accumulated along the particle's path in float64 and added once the trajectories are
    built, before velocity and drift (rounded once; sub-step 0 stays at the start).  Nothing is drawn for it: without the key
    or with all zeros the movie and the truth are the same bit for bit.  truth gains velocity_row [rows, 2] float64.  Together
    with a geometry, confinement or the velocity argument it is a ValueError.  What helpers/msd.segment_transport cuts.

    drift (default None: a stage at rest, the code path without it): the offset of the stage in every frame, a finite real
    [F, 2] array or tensor (y, x) in pixels, or a pair (vy, vx) in pixels per frame for drift[f] = f * (vy, vx).  Row f is added
    to every sub-position of frame f of every particle once the trajectories are built (free, alphas, geometry and states
    alike) and before rendering: truth["pos"] is float32(pos + drift[f]) with the float32 position pos of the stage at rest
    and drift in float64, rounded once, and truth["y"], truth["x"] are the means of those: what was rendered and what a tracker
    sees.  With a geometry truth["arc"] and truth["edge"] stay in the filament's own frame.  truth gains drift ([F, 2]
    float64).  Nothing is drawn for it; a zero drift gives the movie and the positions of drift = None bit for bit.

    camera (default None: the training image model above, the code path without it): a photon-counting camera, a dict
    {"background": photons per pixel, "gain": ADU per photon (default 1), "offset": ADU (default 0), "read_noise": ADU standard
    deviation (default 0)}.  The movie is offset + gain * Poisson(render_movie(pos, amp) + background) + read_noise * randn,
    drawn from `generator` after the amplitudes and the blink draws (randn only with read_noise > 0).  particle_intensity
    keeps its meaning, the peak of the expected image, now in photons; background_intensity and poisson_noise of image_props
    are neither used nor drawn.  truth gains camera (the dict with the defaults filled in) and photons (float64 per row): the
    expected photons of the particle in that frame, amp.sum(-1) * 2 pi (psf_sigma_hr / upsampling_factor)^2.  What
    tracking.fit_spots_mle takes as read_var is (read_noise / gain)^2.

    confinement (default None: free motion, the code path without it): a dict {"radius": a number or [Np] values}, every
    particle diffuses in a harmonic well centred on its start position (an isotropic Ornstein-Uhlenbeck process, _ou_walk
    with a step of 1 / nPosPerFrame frames): radius is the RMS distance from the centre in 2-D in pixels, sqrt(2 s2), and D the
    diffusion coefficient inside the well.  z = randn(Np, T, 2) is drawn where the Brownian steps are and the particle starts
    at the centre.  truth gains radius [Np] float64 and centre [Np, 2] float64 (y, x).  Not together with alphas, geometry or
    states (ValueError); drift moves the wells with the stage.  What helpers/msd.estimate_confinement_ml estimates.

    velocity (default None: no directed motion, the code path without it): a pair (vy, vx) or [Np, 2] values in pixels per
    frame, the constant velocity of every particle on top of its diffusion (motor-driven transport, flow).  velocity * (t /
    nPosPerFrame) is added to sub-position t once the trajectories are built and before drift, in float64, rounded once, the
    way drift is added; truth["y"], truth["x"] are the means of the moved sub-positions.  Nothing is drawn for it; a zero
    velocity gives the movie and the truth of velocity = None bit for bit.  truth gains velocity [Np, 2] float64.  Allowed with
    free motion, alphas and states; with a geometry or confinement it is a ValueError.  helpers/msd.estimate_drift removes
    whatever velocity all tracks share: what helpers/msd.estimate_directed_ml finds after it is each particle's own."""
    props = dict(DEFAULT_IMAGE_PROPS)
    props.update(image_props or {})
    Np, F_, npos, H, W = int(n_particles), int(n_frames), int(nPosPerFrame), int(H), int(W)
    if Np < 0 or F_ < 1 or npos < 1:
        raise ValueError(f"need n_particles >= 0, n_frames >= 1, nPosPerFrame >= 1, got {n_particles}, {n_frames}, {nPosPerFrame}")
    dev = torch.device(device)
    up, sigma = props["upsampling_factor"], psf_sigma_hr(props)
    radius = default_movie_radius(sigma, up)
    margin = float(radius) if margin is None else float(margin)
    if not (margin >= 0 and 2 * margin <= min(H, W) - 1):
        raise ValueError(f"margin = {margin} leaves no room in a field of {H} x {W}")
    if lifetimes is None:
        first = torch.zeros(Np, dtype=torch.int64)
        last = torch.full((Np,), F_ - 1, dtype=torch.int64)
    else:
        lt = torch.as_tensor(lifetimes).detach().cpu()
        if lt.is_floating_point() or tuple(lt.shape) != (Np, 2):
            raise ValueError(f"lifetimes must be integer [{Np}, 2] (first, last), got {tuple(lt.shape)}")
        first, last = lt[:, 0].long(), lt[:, 1].long()
        if bool((first > last).any()):
            raise ValueError("first > last")
        if bool((first < 0).any()) or bool((last >= F_).any()):
            raise ValueError(f"lifetimes must lie in 0 .. {F_ - 1}")
    blink_p = dark = None
    if blink is not None:
        if torch.is_tensor(blink) or isinstance(blink, np.ndarray):
            dark = torch.as_tensor(blink).detach().cpu()
            if dark.dtype != torch.bool or tuple(dark.shape) != (Np, F_):
                raise ValueError(f"a blink mask must be bool [{Np}, {F_}], got {dark.dtype} {tuple(dark.shape)}")
        elif isinstance(blink, bool) or not isinstance(blink, (int, float)) or not 0.0 <= float(blink) < 1.0:
            raise ValueError(f"blink must be a probability in [0, 1) or a bool mask [{Np}, {F_}], got {blink!r}")
        else:
            blink_p = float(blink)
    drift_f = None
    if drift is not None:
        what = f"drift must be a real [{F_}, 2] array or tensor of offsets (y, x) or a pair (vy, vx) in pixels per frame"
        try:
            drift_f = (drift if torch.is_tensor(drift) else torch.from_numpy(np.array(drift))).detach().cpu()     # floats: float64
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{what}, got {drift!r}") from None
        if drift_f.dtype == torch.bool or drift_f.is_complex() or tuple(drift_f.shape) not in ((2,), (F_, 2)):
            raise ValueError(f"{what}, got {drift_f.dtype} {tuple(drift_f.shape)}")
        drift_f = drift_f.double()
        if not bool(torch.isfinite(drift_f).all()):
            raise ValueError("drift must be finite")
        if drift_f.dim() == 1:
            drift_f = torch.arange(F_, dtype=torch.float64).view(F_, 1) * drift_f.view(1, 2)
    vel = None
    if velocity is not None:
        if geometry is not None or confinement is not None:
            raise ValueError("velocity cannot be combined with a geometry or confinement")
        vel = _velocity_matrix(velocity, Np)
    cam = None
    if camera is not None:
        if not isinstance(camera, dict) or "background" not in camera or set(camera) - {"background", "gain", "offset", "read_noise"}:
            raise ValueError("camera must be None or a dict with the key background and optionally gain, offset and read_noise")
        try:
            cam = {k: float(camera.get(k, v)) for k, v in (("background", 0.0), ("gain", 1.0), ("offset", 0.0), ("read_noise", 0.0))}
        except (TypeError, ValueError):
            raise ValueError(f"camera values must be numbers, got {camera!r}") from None
        if not all(math.isfinite(v) for v in cam.values()):
            raise ValueError(f"camera values must be finite, got {camera!r}")
        if cam["background"] < 0 or cam["gain"] <= 0 or cam["read_noise"] < 0:
            raise ValueError(f"camera needs background >= 0, gain > 0 and read_noise >= 0, got {camera!r}")
    gdev = generator.device if generator is not None else dev
    if gdev != dev and not (gdev.type == dev.type and dev.index is None):
        raise ValueError(f"the generator lives on {gdev}, the movie on {dev}")
    packed = None
    if geometry is None:
        if geometry_of is not None or boundary != "clamp":
            raise ValueError("geometry_of and boundary need a geometry")
    else:
        packed, geom_id = _movie_geometries(geometry, geometry_of, boundary, Np, H, W, margin)
    state = state_V = state_V_given = None
    if states is None:
        D = _draw_diffusion_coefficients(Np, Ds, generator, gdev)
    else:
        if alphas is not None:
            raise ValueError("states and alphas cannot be combined: an exponent per state is not supported")
        if Ds is not None:
            raise ValueError("with states the coefficients are states['Ds']: Ds must be None")
        if not isinstance(states, dict) or "Ds" not in states or "M" not in states or set(states) - {"Ds", "M", "p0", "path", "velocity"}:
            raise ValueError("states must be a dict with the keys Ds and M and optionally p0, path and velocity")
        state_Ds, state_M, state_p0 = _markov_args(states["Ds"], states["M"], states.get("p0"))
        if "velocity" in states and states["velocity"] is not None:
            if geometry is not None or confinement is not None or velocity is not None:
                raise ValueError("states['velocity'] cannot be combined with a geometry, confinement or the velocity argument")
            state_V = _state_velocities(states["velocity"], len(state_Ds), "states['velocity']")
            state_V_given = torch.zeros(len(state_Ds), 2, dtype=torch.float64) if state_V is None else state_V
        if states.get("path") is not None:
            path = torch.as_tensor(states["path"]).detach().cpu()
            if path.is_floating_point() or path.dtype == torch.bool or tuple(path.shape) != (Np, F_):
                raise ValueError(f"states['path'] must be integer [{Np}, {F_}], got {path.dtype} {tuple(path.shape)}")
            if path.numel() and (int(path.min()) < 0 or int(path.max()) >= len(state_Ds)):
                raise ValueError(f"states['path'] must lie in [0, {len(state_Ds)})")
            state = path.long().to(gdev)
        else:
            state = markov_states(torch.rand(Np, F_, generator=generator, device=gdev, dtype=torch.float64), state_p0,
                                  state_M).long()
        D_frame = torch.from_numpy(state_Ds).to(gdev)[state]                                                 # [Np, F] float64
    alpha = None if alphas is None else _draw_alphas(Np, alphas, generator, gdev)
    well = None
    if confinement is not None:
        if alphas is not None or geometry is not None or states is not None:
            raise ValueError("confinement cannot be combined with alphas, geometry or states")
        if not isinstance(confinement, dict) or set(confinement) != {"radius"}:
            raise ValueError("confinement must be None or a dict with the key radius")
        well = _radius_vector(confinement["radius"], Np)
    T = F_ * npos
    if state is not None:
        # one factor per sub-step in place of the one per particle: sqrt(2 D / npos) in float32, as without states
        step_scale = torch.sqrt(2.0 * D_frame.float() / npos).repeat_interleave(npos, dim=1).view(Np, T, 1)
    if packed is not None:
        from . import geometry as _geometry
        start = torch.rand(Np, generator=generator, device=gdev).double() * torch.from_numpy(packed["totals"][geom_id]).to(gdev)
        z = torch.randn(Np, T, 1, generator=generator, device=gdev)
        if state is not None:
            steps = z * step_scale
        elif alpha is None:
            steps = z * torch.sqrt(2.0 * D.to(gdev).float() / npos).view(Np, 1, 1)
        else:
            rescale = torch.from_numpy(np.power(float(npos), 1.0 - alpha.numpy())).to(gdev).float()
            steps = fractional_gaussian_noise(z.double(), alpha).float() * torch.sqrt(2.0 * D.to(gdev).float() / npos * rescale).view(Np, 1, 1)
        if T:
            steps[:, 0] = 0.0
        pos64, arc, edge = _geometry.map_displacements(steps.view(Np, T).double(), start, packed, geom_id, boundary, True)
        pos = pos64.float().to(dev)
    else:
        span = torch.tensor([H - 1 - 2 * margin, W - 1 - 2 * margin], device=gdev)
        start = margin + torch.rand(Np, 2, generator=generator, device=gdev) * span
        if well is not None:
            z = torch.randn(Np, T, 2, generator=generator, device=gdev)
            walk = _ou_walk(z.double().transpose(0, 1), D.to(gdev).double(), well.to(gdev), 1.0 / npos, False).transpose(0, 1)
        elif state is not None:
            steps = torch.randn(Np, T, 2, generator=generator, device=gdev) * step_scale
        elif alpha is None:
            steps = torch.randn(Np, T, 2, generator=generator, device=gdev) * torch.sqrt(2.0 * D.to(gdev).float() / npos).view(Np, 1, 1)
        else:
            # variance 2 D / npos^alpha per sub-step, so that a frame of npos sub-steps keeps the MSD 2 D: written as the
            # Brownian variance times npos^(1 - alpha), a factor taken on the host in float64 that is exactly 1 at alpha = 1
            rescale = torch.from_numpy(np.power(float(npos), 1.0 - alpha.numpy())).to(gdev).float()
            z = torch.randn(Np, T, 2, generator=generator, device=gdev)
            steps = fractional_gaussian_noise(z.double(), alpha).float() * torch.sqrt(2.0 * D.to(gdev).float() / npos * rescale).view(Np, 1, 1)
        if well is not None:
            pos = (start.view(Np, 1, 2).double() + walk).float().to(dev)
        else:
            if T:
                steps[:, 0] = 0.0
            pos = (start.view(Np, 1, 2) + torch.cumsum(steps, dim=1)).float().to(dev)
    if state_V is not None:
        # V[state] / npos per sub-step, accumulated along the particle's path in float64 (sub-step 0 stays at the start)
        inc = (state_V.to(dev)[state.to(dev)] / npos).repeat_interleave(npos, dim=1)                          # [Np, T, 2]
        if T:
            inc[:, 0] = 0.0
        pos = (pos.double() + torch.cumsum(inc, dim=1)).float()                                  # rounded once
    if vel is not None:
        vel = vel.to(dev)
        sub = torch.arange(T, dtype=torch.float64, device=dev) / npos
        pos = (pos.double() + vel.view(Np, 1, 2) * sub.view(1, T, 1)).float()                    # rounded once
    if drift_f is not None:
        drift_f = drift_f.to(dev)
        pos = (pos.double() + drift_f.repeat_interleave(npos, dim=0).view(1, T, 2)).float()     # rounded once
    pm, ps = props["particle_intensity"]
    bm, bs = props["background_intensity"]
    if pm > 1e-4 and ps > 1e-4:
        amp = pm / npos + (ps / npos) * torch.randn(Np, F_, npos, generator=generator, device=gdev)
    else:
        amp = torch.zeros(Np, F_, npos, device=gdev)
    amp = amp.float().to(dev)
    if blink is not None:
        if blink_p is not None:
            dark = torch.rand(Np, F_, generator=generator, device=gdev) < blink_p
        dark = dark.to(dev)
        amp = torch.where(dark.unsqueeze(-1), torch.zeros((), dtype=amp.dtype, device=dev), amp)
    vid = render_movie(pos, amp, sigma, H, W, up, radius, first, last).to(dev)
    if cam is None:
        vid = vid + clipped_background(vid.shape, bm, bs, generator, dev)
        pn = props["poisson_noise"]
        if pn != -1:
            vid = vid * torch.poisson(torch.full(vid.shape, float(pn), device=dev), generator=generator) / pn
    else:
        vid = cam["offset"] + cam["gain"] * torch.poisson(vid.float() + cam["background"], generator=generator)
        if cam["read_noise"] > 0:
            vid = vid + cam["read_noise"] * torch.randn(vid.shape, generator=generator, device=dev)
    first, last = first.to(dev), last.to(dev)
    fr = torch.arange(F_, device=dev).view(1, F_)
    pid, frame = ((first.view(Np, 1) <= fr) & (fr <= last.view(Np, 1))).nonzero(as_tuple=True)
    mean_pos = pos.double().view(Np, F_, npos, 2).mean(dim=2)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(last - first + 1, 0)])
    if state is not None:
        state, D_frame = state.to(dev), D_frame.to(dev)
        D_row = D_frame[pid, frame]
        D = torch.zeros(Np, dtype=torch.float64, device=dev).index_add_(0, pid, D_row) / (last - first + 1).double()
    truth = {"frame": frame, "y": mean_pos[pid, frame, 0], "x": mean_pos[pid, frame, 1], "particle_id": pid, "offsets": offsets,
             "D": D.to(dev), "pos": pos, "amp": amp, "first": first, "last": last}
    if state is not None:
        truth["state"], truth["D_row"] = state[pid, frame], D_row
        if state_V_given is not None:
            truth["velocity_row"] = state_V_given.to(dev)[truth["state"]]
    if blink is not None:
        truth["visible"] = ~dark[pid, frame]
    if alpha is not None:
        truth["alpha"] = alpha.to(dev)
    if packed is not None:
        truth["arc"], truth["edge"], truth["geometry_id"] = arc.to(dev), edge.to(dev), torch.from_numpy(geom_id).to(dev)
    if drift_f is not None:
        truth["drift"] = drift_f
    if vel is not None:
        truth["velocity"] = vel
    if well is not None:
        truth["radius"], truth["centre"] = well.to(dev), start.double().to(dev)
    if cam is not None:
        truth["camera"] = cam
        truth["photons"] = amp.double().sum(-1)[pid, frame] * (2.0 * math.pi * (sigma / up) ** 2)
    return vid.float(), truth
