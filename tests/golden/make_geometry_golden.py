#!/usr/bin/env python3
"""Fixture for the filament geometries FROM THE REAL REFERENCE (CPU only):

    python tests/golden/make_geometry_golden.py <reference checkout>

Imports the reference's Experiments/mitochondria_simulation/mitochnodria.py (the `fbm` package is stubbed when it is not
importable: only Edge and Geometry are used; matplotlib likewise) and, for each geometry and displacement case of
tests/geometry_common.py, stores what its Geometry.map_displacements returns; plus, at the probes listed there, its
get_edge_at_length (as edge index, -1 for None, and remainder), Edge.get_position_at_distance, Edge.distance_to_end and
get_edge_at_position (as edge index).  Counts the arc values that land exactly on an interior vertex, asserts there are
enough to pin the tie rule, and stores the count.  Writes tests/golden/geometry/map.npz.  Data only."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) < 2:
    sys.exit(__doc__)
import geometry_common as gc                                        # noqa: E402

try:
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot                                        # noqa: F401
except ImportError:
    sys.modules["matplotlib"] = types.ModuleType("matplotlib")
    sys.modules["matplotlib.pyplot"] = sys.modules["matplotlib"].pyplot = types.ModuleType("matplotlib.pyplot")
try:
    import fbm                                                      # noqa: F401
except ImportError:
    sys.modules["fbm"] = types.ModuleType("fbm")
    sys.modules["fbm"].fgn = None
sys.path.insert(0, os.path.join(os.path.abspath(sys.argv[1]), "Experiments", "mitochondria_simulation"))
import mitochnodria as ref                                          # noqa: E402  (the real reference)

out = {"numpy_version": np.array(np.__version__)}
landings = 0
for name, points in gc.GOLDEN_POINTS.items():
    geom = gc.build(points, ref.Edge, ref.Geometry)
    total = geom.total_length
    out[f"{name}/total"] = np.array(total)
    out[f"{name}/lengths"] = np.array([e.length for e in geom.edges])
    inner = gc.interior_vertex_arcs(points)
    for case, disp, s0 in gc.golden_cases(name, total):
        pos = geom.map_displacements(disp, s0)
        assert pos.shape == (len(disp), 2)
        out[f"{name}/{case}/disp"], out[f"{name}/{case}/s0"], out[f"{name}/{case}/pos"] = disp, np.array(s0), pos
        if case == "int":
            hits = int(np.isin(gc.clamp_walk(disp, s0, total), inner).sum())
            print(f"{name}: {hits} arcs on interior vertices")
            landings += hits
    at, on_edge, where = gc.probes(points, total)
    index = {id(e): i for i, e in enumerate(geom.edges)}
    res = [geom.get_edge_at_length(float(d)) for d in at]
    out[f"{name}/at_length_edge"] = np.array([-1 if e is None else index[id(e)] for e, _ in res], np.int64)
    out[f"{name}/at_length_rem"] = np.array([r for _, r in res], np.float64)
    out[f"{name}/position_at_distance"] = np.array([geom.edges[e].get_position_at_distance(d) for e, d in on_edge])
    out[f"{name}/distance_to_end"] = np.array([[geom.edges[e].distance_to_end(w) for w in where] for e in range(len(geom.edges))])
    found = [geom.get_edge_at_position(w) for w in where]
    out[f"{name}/at_position_edge"] = np.array([-1 if e is None else index[id(e)] for e in found], np.int64)
assert landings >= 20, landings
out["vertex_landings"] = np.array(landings)

os.makedirs(gc.GOLDEN_DIR, exist_ok=True)
np.savez_compressed(gc.GOLDEN, **out)
print(f"{gc.GOLDEN}: {os.path.getsize(gc.GOLDEN) / 1024:.0f} KiB, {landings} vertex landings")
