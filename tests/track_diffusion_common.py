"""Shared by tests/test_track_diffusion.py, tests/test_track_diffusion_gpu.py and tests/golden/make_track_diffusion_golden.py:
the seeded ragged tracks of the fixture tests/golden/track_diffusion/msd.npz and the bars of the per-track diffusion
estimates, with their origin.

The bars
  MSD_RTOL.  The numpy statement of track_msd (helpers/msd.py) and the reference (helpers/helpersMSD.py) compute the same
  quantities and differ only in the order of their sums: np.mean / a BLAS product / an SVD against one ascending sum.  Every
  sum has at most 256 non-negative fp64 terms (the longest track has 257 rows), so the two differ by about
  256 * 2.2e-16 = 6e-14 relative; 1e-12 leaves a factor 17.
  The kernel performs the operations of the numpy statement in its order without contraction: it is held bitwise.
  Refined positions come from the Gaussian fit, which the kernel is held to at 1e-9 relative (tracking_common.KERNEL_FIT_RTOL);
  what is computed from them is held to the same bar."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_diffusion")
GOLDEN = os.path.join(GOLDEN_DIR, "msd.npz")

LENGTHS = [1, 2, 3, 5, 30, 63, 64, 65, 257]
DT = 0.03
SEED = 20251
MAX_LAG = 4
MSD_RTOL = 1e-12


def tracks():
    """Seeded Brownian tracks of LENGTHS rows, concatenated -> (positions [N, 2] float64 (y, x), offsets [n + 1] int64)."""
    rng = np.random.default_rng(SEED)
    parts = []
    for k, L in enumerate(LENGTHS):
        start = rng.uniform(20.0, 100.0, (1, 2))
        parts.append(start + np.cumsum(rng.normal(0.0, 0.4 + 0.15 * k, (L, 2)), axis=0))
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)


def long_tracks(lengths, seed=5):
    """Seeded tracks of arbitrary lengths (both sides of the LDS cap of csrc/diffusion.hip)."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([rng.uniform(0.0, 500.0, (1, 2)) + np.cumsum(rng.normal(0.0, 0.7, (L, 2)), axis=0) for L in lengths])
    return pos, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def load():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def same_bits(a, b):
    """Bitwise equality of two float arrays, NaN positions included (any NaN equals any NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(np.isnan(a), np.isnan(b))) and \
        bool(np.array_equal(np.where(np.isnan(a), 0, a).view(np.uint64 if a.dtype == np.float64 else np.uint32),
                            np.where(np.isnan(b), 0, b).view(np.uint64 if b.dtype == np.float64 else np.uint32)))
