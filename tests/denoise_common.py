"""Shared by tests/test_denoise.py, tests/test_denoise_gpu.py and tests/golden/make_denoise_golden.py: fixed 9x9 frames in
the normalised range of trajs_to_vid_norm_rl, an asymmetric PSF, and the bars RL-TV is held to against the reference.

The bars: the restatement sums the convolutions directly, the reference through float64 FFTs (~1e-16 apart).  With
tv_weight = 0 that stays below 1e-6 at every snapshot.  With a TV term, sqrt(dx^2 + dy^2 + 1e-8) acts as a sign function
near flat or clipped regions and amplifies the reference's own float32 rounding flips by up to ~1e4 by iteration 11, so
only the early snapshots are held per pixel; the later ones are held to a quantile and a loose maximum."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise", "rl_tv.npz")
ALL_TV0 = 1e-6
EARLY_TV = 1e-5            # snapshots after iteration <= 2 with a TV term
LATE_TV_Q = (0.99, 1e-4)   # later snapshots: >= 99 % of pixels within 1e-4 ...
LATE_TV_MAX = 1e-2         # ... and all within 1e-2
GAUSS_FILTER_ULPS = 1      # Gaussian filter, kernel against restatement and scipy: the last float32 bit (fp64 sums in another order)


def frames_9x9(n, seed=1234, size=9):
    """Background ~ N(0.07, 0.07) plus one Gaussian spot of amplitude ~0.9 near the centre, float32 [n, size, size]."""
    rng = np.random.default_rng(seed)
    ax = np.arange(size, dtype=np.float64) - (size - 1) / 2
    x, y = np.meshgrid(ax, ax)
    cx, cy = rng.uniform(-2, 2, (2, n, 1, 1))
    s = rng.uniform(0.8, 1.6, (n, 1, 1))
    amp = rng.normal(0.9, 0.12, (n, 1, 1))
    spot = amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return (spot + rng.normal(0.07, 0.07, (n, size, size))).astype(np.float32)


def asymmetric_psf(size=9):
    """A non-negative PSF with no mirror symmetry: pins the orientation of both convolutions."""
    ax = np.arange(size, dtype=np.float64) - (size - 1) / 2
    x, y = np.meshgrid(ax, ax)
    p = np.exp(-((x - 0.7) ** 2 / (2 * 1.1 ** 2) + (y + 0.4) ** 2 / (2 * 0.8 ** 2))) * (1.0 + 0.3 * (x > 0) + 0.1 * (y > 1))
    return p / p.sum()


def check_rl_bars(got, ref, its, tv_weight):
    """got / ref [n, len(its), H, W]; returns (failure messages, stats)."""
    msgs = []
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    stats = {"max": float(err.max()) if err.size else 0.0}
    for k, it in enumerate(its):
        e = err[:, k].ravel()
        if tv_weight == 0:
            if e.max() > ALL_TV0:
                msgs.append(f"tv 0, iteration {it}: max {e.max():.2e} > {ALL_TV0}")
        elif it <= 2:
            if e.max() > EARLY_TV:
                msgs.append(f"tv {tv_weight}, iteration {it}: max {e.max():.2e} > {EARLY_TV}")
        else:
            frac = float(np.mean(e <= LATE_TV_Q[1]))
            if frac < LATE_TV_Q[0] or e.max() > LATE_TV_MAX:
                msgs.append(f"tv {tv_weight}, iteration {it}: {frac:.4f} within {LATE_TV_Q[1]}, max {e.max():.2e}")
    return msgs, stats
