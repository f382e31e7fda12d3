#!/usr/bin/env python3
"""Fixture for the per-track MSD estimates FROM THE REAL REFERENCE (CPU only):

    python tests/golden/make_track_diffusion_golden.py <reference checkout>

Imports the reference's helpers/helpersMSD.py (matplotlib is stubbed when it is not importable: nothing is plotted) and
applies, to each of the seeded ragged tracks of tests/track_diffusion_common.py, its mean_square_displacement,
estimateDfromMSDs(msd[None], arange(L) * dt) and estimateDfromMSDsWeighted, and the two estimators again on the first
MAX_LAG + 1 entries of the MSD (what track_msd(max_lag=MAX_LAG) is compared with).  Stores positions, offsets and results in
tests/golden/track_diffusion/msd.npz.  Data only."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) < 2:
    sys.exit(__doc__)
import track_diffusion_common as dc                                 # noqa: E402

try:
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot                                        # noqa: F401
except ImportError:
    sys.modules["matplotlib"] = types.ModuleType("matplotlib")
    sys.modules["matplotlib.pyplot"] = sys.modules["matplotlib"].pyplot = types.ModuleType("matplotlib.pyplot")
sys.path.insert(0, os.path.abspath(sys.argv[1]))
from helpers import helpersMSD as ref                               # noqa: E402  (the real reference)

pos, offsets = dc.tracks()
n = len(dc.LENGTHS)
Lmax = max(dc.LENGTHS)
msd = np.zeros((n, Lmax))
est = {k: np.zeros(n) for k in ("d_lstsq", "d_weighted", "d_lstsq_max_lag", "d_weighted_max_lag")}
for k, L in enumerate(dc.LENGTHS):
    m = ref.mean_square_displacement(pos[offsets[k]:offsets[k + 1]])
    assert m.shape == (L,)
    msd[k, :L] = m
    for suffix, cut in (("", L), ("_max_lag", min(L, dc.MAX_LAG + 1))):
        time_range = np.arange(cut) * dc.DT
        est["d_lstsq" + suffix][k] = ref.estimateDfromMSDs(m[None, :cut], time_range)[0]
        est["d_weighted" + suffix][k] = ref.estimateDfromMSDsWeighted(m[None, :cut], time_range)[0]
    print(f"track {k}: {L} rows, D_lstsq {est['d_lstsq'][k]:.6g}, D_weighted {est['d_weighted'][k]:.6g}")

os.makedirs(dc.GOLDEN_DIR, exist_ok=True)
np.savez_compressed(dc.GOLDEN, numpy_version=np.array(np.__version__), lengths=np.array(dc.LENGTHS, np.int64),
                    dt=np.array(dc.DT), max_lag=np.array(dc.MAX_LAG), positions=pos, offsets=offsets, msd=msd, **est)
print(f"{dc.GOLDEN}: {os.path.getsize(dc.GOLDEN) / 1024:.0f} KiB")
