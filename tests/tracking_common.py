"""Shared by tests/test_tracking.py, tests/test_tracking_gpu.py, tests/golden/make_tracking_golden.py and
scripts/bench_tracking.py: seeded synthetic movies, the plain numpy statement of skimage.feature.peak_local_max that the
fixture was made with, and the bars the tracking front end is held to, with their origin.

The bars
  DoG.  The restatement (helpers/tracking._dog_numpy) sums in scipy.ndimage.correlate1d's order and rounds each pass to float32
  as scipy does, so it is held bitwise to scipy.ndimage.gaussian_filter: measured equal on all fixture movies and on 1 000
  random frames (tests/golden/make_tracking_golden.py repeats the measurement whenever the fixture is rebuilt, and
  tests/test_tracking.py on every run for a smaller sample).  DOG_BAR_ULP = 0; the kernel is held bitwise to the restatement.
  The fixture's margins (every peak above the threshold, above the strongest value it beat, every rejected candidate below
  the threshold) are asserted to be at least MARGIN_FACTOR x one float32 ulp at the frame's maximum, so that a last-bit
  difference in a filter could not change the peak set.
  Fit.  The reference's curve_fit is MINPACK's lmdif with a finite-difference Jacobian stopped at ftol = xtol = 1.49e-8, so its
  answer lies at some distance from the least-squares optimum.  FIT_MEASURED is, per parameter the reference returns (x0, y0, sigma),
  the largest |reference - restatement run to xtol = 1e-13| over all fits of the fixture; FIT_BAR = 4 x that (the
  factor covers patches of later fixtures that condition worse than the ones sampled).  The kernel evaluates exp() with the
  device's library, not the host's, so it is not bitwise: it is held to the restatement at KERNEL_FIT_RTOL = 1e-9 relative,
  the level the trajectory descriptors are pinned at."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking")
GOLDEN = os.path.join(GOLDEN_DIR, "tracking.npz")

DOG_BAR_ULP = 0
MARGIN_FACTOR = 100
# measured by make_tracking_golden.py on the 423 fits of the fixture (x0, y0 in pixels, sigma in pixels).  The reference
# returns only these three of the five parameters (x_refined, y_refined, psf_size), so only they can be held against it.
FIT_MEASURED = {"x0": 8.90464659e-05, "y0": 1.19918724e-05, "sigma": 1.61656710e-05}
FIT_BAR = {k: 4.0 * v for k, v in FIT_MEASURED.items()}
KERNEL_FIT_RTOL = 1e-9
PATCH_SIZE = 9

# name -> (seed, frames, H, W, particles, amplitude, spot sigma, background, step)
MOVIES = {
    "main": (7, 30, 128, 128, 12, 200.0, 1.3, 20.0, 1.0),
    "odd": (11, 8, 97, 141, 9, 150.0, 1.1, 10.0, 1.5),
}


def synthetic_movie(seed, frames, H, W, particles, amplitude=200.0, spot_sigma=1.3, background=20.0, step=1.0, margin=10):
    """Gaussian spots on Brownian paths over a constant background with Poisson noise, float32 [frames, H, W]."""
    rng = np.random.default_rng(seed)
    start = np.stack([rng.uniform(margin, H - margin, particles), rng.uniform(margin, W - margin, particles)], axis=1)
    pos = start[None] + np.cumsum(rng.normal(0.0, step, (frames, particles, 2)), axis=0)
    yy, xx = np.mgrid[0:H, 0:W]
    mov = np.zeros((frames, H, W))
    for f in range(frames):
        for p in range(particles):
            mov[f] += amplitude * np.exp(-((yy - pos[f, p, 0]) ** 2 + (xx - pos[f, p, 1]) ** 2) / (2 * spot_sigma ** 2))
    return rng.poisson(mov + background).astype(np.float32)


def movie(name):
    return synthetic_movie(*MOVIES[name])


def spot_patches(n, P, seed=3, amplitude=200.0, background=20.0, noise=True):
    """n patches of side P with one Gaussian spot near the centre, float32."""
    rng = np.random.default_rng(seed)
    ax = np.arange(P, dtype=np.float64)
    x, y = np.meshgrid(ax, ax)
    cx, cy = rng.uniform(P // 2 - 0.8, P // 2 + 0.8, (2, n, 1, 1))
    s = rng.uniform(0.9, 1.6, (n, 1, 1))
    a = rng.uniform(0.6, 1.4, (n, 1, 1)) * amplitude
    img = background + a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return (rng.poisson(img) if noise else img).astype(np.float32)


def peak_local_max(image, min_distance=1, threshold_abs=None, exclude_border=True):
    """What skimage.feature.peak_local_max(image, min_distance, threshold_abs, exclude_border=False) is taken to compute
    (skimage is not available where the fixture is made): window maxima with replicated borders, none on a flat image, strictly
    above the threshold, strongest first with ties in row-major order, then greedy spacing by Chebyshev distance."""
    from scipy import ndimage
    assert exclude_border is False
    mask = image == ndimage.maximum_filter(image, size=2 * min_distance + 1, mode="nearest")
    if np.all(mask):
        mask[:] = False
    mask &= image > threshold_abs
    coords = np.nonzero(mask)
    coords = np.transpose(coords)[np.argsort(-image[coords], kind="stable")]
    keep = []
    for p in coords:
        if all(np.max(np.abs(p - q)) > min_distance for q in keep):
            keep.append(p)
    return np.array(keep, dtype=np.int64).reshape(-1, 2)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))
