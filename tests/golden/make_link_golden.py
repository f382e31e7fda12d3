#!/usr/bin/env python3
"""Fixture for linking FROM THE REAL REFERENCE (CPU only):

    python tests/golden/make_link_golden.py <reference checkout>

Imports the reference's helpers/helpersTracking.py with the stub plotting / skimage modules make_tracking_golden.py uses,
calls its link_particles on every pair of consecutive frames of the seeded sequences of tests/linking_common.py, repeats each
call under ORDER_PERMUTATIONS random permutations of rows and columns to flag the pairs whose link set does not depend on
the order, asserts the bound on order-dependent pairs, and stores coordinates, links and flags in
tests/golden/tracking_link/link.npz.  Data only."""
import os
import sys
import types

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) < 2:
    sys.exit(__doc__)
import linking_common as lc                                         # noqa: E402

for name in ("skimage", "skimage.feature", "IPython", "IPython.display", "seaborn"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["skimage.feature"].peak_local_max = None
sys.modules["IPython.display"].HTML = None
sys.modules["IPython.display"].display = None
import matplotlib                                                   # noqa: E402

matplotlib.use("Agg")
sys.path.insert(0, os.path.abspath(sys.argv[1]))
from helpers import helpersTracking as ref                          # noqa: E402  (the real reference)


def reference_links(c0, c1):
    links, _, _ = ref.link_particles(c0, c1, max_distance=lc.MAX_DISTANCE)
    return {(int(i), int(j)) for i, j in links}


out = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__),
       "max_distance": np.array(lc.MAX_DISTANCE), "order_permutations": np.array(lc.ORDER_PERMUTATIONS)}
all_cases = lc.cases()
out["cases"] = np.array(list(all_cases))
perm_rng = np.random.default_rng(2025)
for name, frames in all_cases.items():
    rows, flags = [], []
    for p in range(len(frames) - 1):
        c0, c1 = frames[p], frames[p + 1]
        base = reference_links(c0, c1)
        same = True
        for _ in range(lc.ORDER_PERMUTATIONS):
            p0, p1 = perm_rng.permutation(len(c0)), perm_rng.permutation(len(c1))
            same = same and {(int(p0[i]), int(p1[j])) for i, j in reference_links(c0[p0], c1[p1])} == base
        rows += [(p, i, j) for i, j in sorted(base)]
        flags.append(same)
    flags = np.array(flags, bool)
    false_fraction = float((~flags).mean())
    print(f"{name}: {len(frames)} frames, {len(rows)} links, {int((~flags).sum())} of {len(flags)} pairs order dependent")
    if name in lc.BOUNDED:
        assert false_fraction <= lc.MAX_FALSE_FRACTION, (name, false_fraction)
    out[f"{name}_counts"] = np.array([len(c) for c in frames], np.int32)
    out[f"{name}_coords"] = np.concatenate(frames).astype(np.int16)
    assert np.array_equal(out[f"{name}_coords"], np.concatenate(frames))
    out[f"{name}_links"] = np.array(rows, np.int16).reshape(-1, 3)
    assert np.array_equal(out[f"{name}_links"], np.array(rows, np.int64).reshape(-1, 3))
    out[f"{name}_order_independent"] = flags

os.makedirs(lc.GOLDEN_DIR, exist_ok=True)
np.savez_compressed(lc.GOLDEN, **out)
print(f"{lc.GOLDEN}: {os.path.getsize(lc.GOLDEN) / 1024:.0f} KiB")
