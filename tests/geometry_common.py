"""Shared by tests/test_geometry.py, tests/test_geometry_gpu.py and tests/golden/make_geometry_golden.py: the geometries and
displacement cases, a point-to-polyline distance, the exact per-step oracle of the reflecting walk in fractions.Fraction and
the bound the float64 walk is held to.

Bound of the reflecting walk, |s_float - s_exact| <= 2 T ulp(max|d| + 2 total): a step takes one rounding in s + d and at
most one in m + P (fmod is exact, and P - m is exact for L < m <= P), each at most half an ulp of a number no larger than
max|d| + 2 total; the reflection is 1-Lipschitz, so errors add and never grow: T ulp in all.  The factor 2 is margin."""
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "geometry")
GOLDEN = os.path.join(GOLDEN_DIR, "map.npz")

# golden geometries: exactly representable edge lengths only, so bitwise equality does not depend on the numpy build
GOLDEN_POINTS = {
    # the notebook's ten-edge serpentine, total length 1550
    "serpentine": [(0, 300), (0, 0), (100, 0), (100, 200), (130, 200), (130, 0), (230, 0), (230, 250), (260, 250), (260, 0),
                   (350, 0)],
    "pythagorean": [(0, 0), (30, 40), (30, 100), (-18, 164)],             # edges 50, 60, 80
    "single": [(2, 1), (14, 6)],                                          # one edge of 13
}
GOLDEN_T = 400
GOLDEN_SCALES = (0.01, 0.3, 1.5)                                          # sigma of the seeded normals, in total lengths


def build(points, Edge, Geometry):
    """A chain through `points` from the given classes (the project's or the reference's)."""
    return Geometry([Edge(a, b) for a, b in zip(points[:-1], points[1:])])


def golden_cases(name, total):
    """name -> list of (case, disp [T] float64, start): seeded normals at three scales with starts below 0, beyond the total, 0
    and the total, and one integer-valued sequence (multiples of 10) from an integer start that lands on vertices."""
    rng = np.random.default_rng(sorted(GOLDEN_POINTS).index(name) + 100)
    starts = (-0.25 * total, 1.5 * total, 0.0, float(total))
    cases = []
    for i, scale in enumerate(GOLDEN_SCALES):
        for j, s0 in enumerate(starts):
            cases.append((f"s{i}_{j}", rng.standard_normal(GOLDEN_T) * scale * total, s0))
    span = max(1, int(total // 40))
    cases.append(("int", rng.integers(-span, span + 1, size=4 * GOLDEN_T).astype(np.float64) * 10.0, 70.0))
    return cases


def clamp_walk(disp, s0, total):
    """the clamped arc in plain Python, as the reference's loop takes it"""
    s = max(0, min(s0, total))
    out = []
    for d in disp:
        s = max(0, min(s + d, total))
        out.append(s)
    return np.array(out, dtype=np.float64)


def interior_vertex_arcs(points):
    """cumulative lengths at the interior vertices (exact for the golden geometries)"""
    p = np.asarray(points, dtype=np.float64)
    return np.cumsum(np.linalg.norm(p[1:] - p[:-1], axis=1))[:-1]


def probes(points, total):
    """(lengths probed by get_edge_at_length, (edge, distance) pairs probed by get_position_at_distance / distance_to_end,
    points probed by get_edge_at_position)"""
    inner = interior_vertex_arcs(points)
    at = np.concatenate([[-1.0, 0.0, total, total + 1.0, 0.5 * total, total / 3.0], inner, inner + 0.25, inner - 0.25])
    n_edges = len(points) - 1
    on_edge = [(e, d) for e in range(n_edges) for d in (-1.0, 0.0, 0.375, 7.0, 1e9)]
    p = np.asarray(points, dtype=np.float64)
    mid = 0.5 * (p[1:] + p[:-1])
    where = np.concatenate([p, mid, mid + np.array([0.0, 1e-3]), mid + np.array([1e-12, 0.0]), p + 1000.0])
    return at, on_edge, where


def random_geometry(n_edges, seed, step=7.0):
    """points of a chain of n_edges edges with real vertices: a random walk in the plane with steps of 0.5 .. 1.5 `step`"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n_edges)
    r = rng.uniform(0.5, 1.5, n_edges) * step
    pts = np.concatenate([[[3.25, -1.5]], np.array([3.25, -1.5]) + np.cumsum(np.stack([r * np.cos(ang), r * np.sin(ang)], 1), 0)])
    return [tuple(p) for p in pts]


# (edges, seed) of random_geometry chains on which the sequential subtraction of the edge lengths from s = total leaves a
# remainder a few ulps ABOVE the last length, so that no edge is found: the branch the reference answers with its last end
# point.  Which chains do is an accident of rounding (about two in five of the seeded ones); open_end_remainder checks it.
OPEN_END = ((2, 3), (4, 3), (13, 0))


def open_end_remainder(lengths, total):
    """what is left of `total` after subtracting every edge length but the last, one by one, as get_edge_at_length does"""
    rem = total
    for le in lengths[:-1]:
        if rem <= le:
            return None                                                   # an earlier edge takes it
        rem = rem - le
    return rem


def batch(N, T, totals, seed):
    """disp [N, T], s0 [N], geom_of [N] for len(totals) geometries: unsorted geom_of with repeats, step scales from 0.01 to 2
    total lengths per particle (so some steps exceed the total), every fourth start outside [0, total]"""
    rng = np.random.default_rng(seed)
    G = len(totals)
    geom_of = rng.permutation(np.arange(N) % G).astype(np.int64) if N >= G else rng.integers(0, G, N)
    L = np.asarray(totals, dtype=np.float64)[geom_of]
    scale = np.array([0.01, 0.1, 0.5, 2.0])[np.arange(N) % 4] * L
    disp = rng.standard_normal((N, T)) * scale[:, None]
    s0 = rng.uniform(0, 1, N) * L
    s0[::4] = np.where(np.arange(N)[::4] % 8 == 0, -0.3 * L[::4], 1.7 * L[::4])
    return disp, s0, geom_of


def polyline_distance(p, verts):
    """distance of every point p [..., 2] to the polyline through verts [V, 2] (float64)"""
    p = np.asarray(p, dtype=np.float64)[..., None, :]
    a, b = verts[:-1], verts[1:]
    ab = b - a
    t = np.clip(((p - a) * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    return np.sqrt((((a + t[..., None] * ab) - p) ** 2).sum(-1)).min(-1)


def reflect_oracle(disp, s0, total):
    """the reflecting walk of one particle in exact rational arithmetic: every step the position is reflected at 0 and at
    `total` (as often as needed) -> list of Fraction, the arc after each step"""
    L = Fraction(float(total))
    P = 2 * L

    def fold(m):
        m = m % P                                                         # Python's %: in [0, P)
        return P - m if m > L else m

    s = fold(Fraction(float(s0)))
    out = []
    for d in disp:
        s = fold(s + Fraction(float(d)))
        out.append(s)
    return out


def reflect_bound(T, disp, total):
    return 2.0 * T * float(np.spacing(np.abs(disp).max() + 2.0 * total))


def reflect_error(arc, disp, s0, total):
    """max |arc - oracle| over the steps, as a float"""
    want = reflect_oracle(disp, s0, total)
    return float(max(abs(Fraction(float(a)) - w) for a, w in zip(arc, want)))


REFLECT_TS = (1, 64, 257)
REFLECT_TOTALS = (1e-3, 7.3, 1550.0)
REFLECT_SCALES = (0.01, 0.3, 1.0, 40.0)


def reflect_cases():
    """[(T, total, scale, disp [T], s0)]: every length, total and step scale, starts inside and outside"""
    rng = np.random.default_rng(2024)
    out = []
    for T in REFLECT_TS:
        for total in REFLECT_TOTALS:
            for k, scale in enumerate(REFLECT_SCALES):
                s0 = (0.3 * total, -2.6 * total, 5.2 * total, total)[k]
                out.append((T, total, scale, rng.standard_normal(T) * scale * total, s0))
    return out


PROPS = {"upsampling_factor": 3}
OLD_KEYS = {"frame", "y", "x", "particle_id", "offsets", "D", "pos", "amp", "first", "last"}


def movie_geometries():
    """two serpentines inside a 40 x 48 field (margin 9 at up-sampling 3)"""
    from moleculardiffusion_mivit_amd.helpers import geometry as geo
    return [geo.cristae_geometry(2, 6.0, 8.0, 3.0, lead=4.0, origin=(10.0, 10.0)),
            geo.cristae_geometry(1, 1.0, 12.0, 10.0, lead=3.0, origin=(12.0, 14.0))]


def check_movie(movie, truth, geoms, alphas, device):
    """what simulate_movie(5, 6, 40, 48, ..., 4, geometry=geoms) must return, on either device"""
    import torch
    from moleculardiffusion_mivit_amd.helpers import geometry as geo
    Np, F, npos = 5, 6, 4
    extra = {"arc", "edge", "geometry_id"} | ({"alpha"} if alphas is not None else set())
    assert set(truth) == OLD_KEYS | extra
    assert movie.shape == (F, 40, 48) and movie.dtype == torch.float32 and movie.device.type == device
    assert truth["arc"].shape == (Np, F * npos) and truth["arc"].dtype == torch.float64
    assert truth["edge"].shape == (Np, F * npos) and truth["edge"].dtype == torch.int32
    assert truth["geometry_id"].dtype == torch.int64 and truth["geometry_id"].tolist() == [0, 1, 0, 1, 0]
    assert truth["pos"].dtype == torch.float32 and all(v.device.type == device for v in truth.values())
    pos, arc, edge = truth["pos"].cpu().numpy(), truth["arc"].cpu().numpy(), truth["edge"].cpu().numpy()
    for k, g in enumerate(geoms):
        mine = truth["geometry_id"].cpu().numpy() == k
        d = polyline_distance(pos[mine][..., ::-1], geo.pack_geometries(g)["verts"])       # pos is (y, x)
        print(f"geometry {k}: farthest sub-position {d.max():.3g} px off the filament")
        assert d.max() <= 1e-4
        assert (arc[mine] >= 0).all() and (arc[mine] <= g.total_length).all()
        assert (edge[mine] >= 0).all() and (edge[mine] < len(g.edges)).all()
    assert bool(torch.isfinite(movie).all())
