"""CPU: helpers/geometry.py, the mirror of the reference's filament geometry, and the numpy restatement of csrc/confine.hip.
Clamp mode is held BITWISE against what the real reference returned (tests/golden/geometry/map.npz, made by
tests/golden/make_geometry_golden.py); the reflecting mode against the exact per-step oracle of tests/geometry_common.py
within the bound derived there; then the batched and multi-geometry forms, non-finite steps, every ValueError, disp_fbm,
cristae_geometry and simulate_movie(geometry=...)."""
import numpy as np
import pytest
import torch

import geometry_common as gc
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import geometry as geo


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(gc.GOLDEN))


def _geom(name):
    return gc.build(gc.GOLDEN_POINTS[name], geo.Edge, geo.Geometry)


@pytest.mark.parametrize("name", sorted(gc.GOLDEN_POINTS))
def test_mirror_classes_match_the_reference_bitwise(golden, name):
    g = _geom(name)
    points = gc.GOLDEN_POINTS[name]
    assert np.array_equal(bits(g.total_length), bits(golden[f"{name}/total"]))
    assert np.array_equal(bits([e.length for e in g.edges]), bits(golden[f"{name}/lengths"]))
    at, on_edge, where = gc.probes(points, g.total_length)
    index = {id(e): i for i, e in enumerate(g.edges)}
    res = [g.get_edge_at_length(float(d)) for d in at]
    assert [-1 if e is None else index[id(e)] for e, _ in res] == golden[f"{name}/at_length_edge"].tolist()
    assert np.array_equal(bits([r for _, r in res]), bits(golden[f"{name}/at_length_rem"]))
    got = np.array([g.edges[e].get_position_at_distance(d) for e, d in on_edge])
    assert np.array_equal(bits(got), bits(golden[f"{name}/position_at_distance"]))
    got = np.array([[g.edges[e].distance_to_end(w) for w in where] for e in range(len(g.edges))])
    assert np.array_equal(bits(got), bits(golden[f"{name}/distance_to_end"]))
    found = [g.get_edge_at_position(w) for w in where]
    assert [-1 if e is None else index[id(e)] for e in found] == golden[f"{name}/at_position_edge"].tolist()
    for a, b in zip(g.edges[:-1], g.edges[1:]):
        assert a.ancestor is b and b.predecessor is a
    assert g.edges[0].predecessor is None and g.edges[-1].ancestor is None
    p = np.asarray(points, dtype=np.float64)
    assert (g.min_x, g.max_x, g.min_y, g.max_y) == (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max())
    assert repr(g) == f"Geometry(edges={len(points) - 1}, total_length={g.total_length:.2f})"
    assert repr(g.edges[0]).startswith("Edge(start=(") and "angle=" in repr(g.edges[0])


@pytest.mark.parametrize("name", sorted(gc.GOLDEN_POINTS))
def test_restatement_matches_the_reference_bitwise(golden, name):
    g = _geom(name)
    cases = gc.golden_cases(name, g.total_length)
    for case, disp, s0 in cases:
        assert np.array_equal(bits(disp), bits(golden[f"{name}/{case}/disp"])), "the fixture is stale"
        got = g.map_displacements(disp, s0)
        assert got.shape == (len(disp), 2) and got.dtype == np.float64
        assert np.array_equal(bits(got), bits(golden[f"{name}/{case}/pos"])), (name, case)
    # the batched form, row by row (equal lengths only: the integer case is longer)
    same = [c for c in cases if len(c[1]) == gc.GOLDEN_T]
    disp, s0 = np.stack([c[1] for c in same]), np.array([c[2] for c in same])
    got = g.map_displacements(disp, s0)
    assert got.shape == (len(same), gc.GOLDEN_T, 2)
    for k, (case, _, _) in enumerate(same):
        assert np.array_equal(bits(got[k]), bits(golden[f"{name}/{case}/pos"])), (name, case)
    got_t = g.map_displacements(torch.from_numpy(disp), torch.from_numpy(s0))
    assert torch.is_tensor(got_t) and np.array_equal(bits(got_t.numpy()), bits(got))


def test_the_tie_rule_is_exercised(golden):
    assert int(golden["vertex_landings"]) >= 20
    hits = 0
    for name, points in gc.GOLDEN_POINTS.items():
        g = _geom(name)
        case, disp, s0 = gc.golden_cases(name, g.total_length)[-1]
        assert case == "int"
        _, arc, edge = geo.map_displacements(disp[None], s0, g, return_arc_edge=True)
        assert np.array_equal(bits(arc[0]), bits(gc.clamp_walk(disp, s0, g.total_length)))
        inner = gc.interior_vertex_arcs(points)
        on = np.isin(arc[0], inner)
        hits += int(on.sum())
        assert np.array_equal(edge[0][on], np.searchsorted(inner, arc[0][on]))    # the EARLIER edge wins at a vertex
    assert hits == int(golden["vertex_landings"])


def test_several_geometries_with_an_unsorted_assignment_equal_each_alone():
    geoms = [gc.build(gc.random_geometry(E, seed=E), geo.Edge, geo.Geometry) for E in (13, 1, 2)]
    disp, s0, geom_of = gc.batch(37, 65, [g.total_length for g in geoms], seed=5)
    assert not np.array_equal(geom_of, np.sort(geom_of))
    for boundary in geo.BOUNDARIES:
        pos, arc, edge = geo.map_displacements(disp, s0, geoms, geom_of, boundary, return_arc_edge=True)
        assert pos.shape == (37, 65, 2) and arc.shape == (37, 65) and edge.dtype == np.int32
        for n in range(37):
            g = geoms[geom_of[n]]
            p1, a1, e1 = geo.map_displacements(disp[n:n + 1], s0[n:n + 1], g, boundary=boundary, return_arc_edge=True)
            assert np.array_equal(bits(p1[0]), bits(pos[n])) and np.array_equal(bits(a1[0]), bits(arc[n]))
            assert np.array_equal(e1[0], edge[n])
            assert np.array_equal(bits(g.map_displacements(disp[n], s0[n], boundary=boundary)), bits(pos[n]))
        assert (arc >= 0).all() and (arc <= np.array([g.total_length for g in geoms])[geom_of][:, None]).all()
        for k, g in enumerate(geoms):
            d = gc.polyline_distance(pos[geom_of == k], geo.pack_geometries(g)["verts"])
            assert d.max() <= 1e-9 * g.total_length
    # the default assignment is round robin
    got = geo.map_displacements(disp, s0, geoms)
    want = geo.map_displacements(disp, s0, geoms, np.arange(37) % 3)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("n_edges,seed", gc.OPEN_END)
def test_no_edge_found_gives_the_last_vertex_and_the_last_edge(n_edges, seed):
    """real vertices: at s = total the remainder ends above the last length, the reference's get_edge_at_length finds no edge
    and its map_displacements answers with the last end point; steps larger than the total clamp s to the total"""
    g = gc.build(gc.random_geometry(n_edges, seed), geo.Edge, geo.Geometry)
    total, lens = g.total_length, [e.length for e in g.edges]
    rem = gc.open_end_remainder(lens, total)
    assert rem is not None and rem > lens[-1]
    assert g.get_edge_at_length(total) == (None, 0)                           # the mirror class takes the reference's branch
    disp, s0, geom_of = gc.batch(37, 65, [total], seed=n_edges)
    last = np.asarray(g.edges[-1].end_point)
    for boundary in geo.BOUNDARIES:
        pos, arc, edge = geo.map_displacements(disp, s0, g, geom_of, boundary, True)
        open_ = arc == total
        print(f"{n_edges} edges, {boundary}: {int(open_.sum())} samples find no edge")
        if boundary == "clamp":
            assert open_.sum() > 0
        assert np.array_equal(bits(pos[open_]), bits(np.broadcast_to(last, pos[open_].shape)))
        assert (edge[open_] == n_edges - 1).all()
        # one step below the total an edge is found again and the position is interpolated, not the vertex
        near = geo.map_displacements(np.array([[-1e-3]]), total, g, boundary=boundary, return_arc_edge=True)
        assert near[2][0, 0] == n_edges - 1 and not np.array_equal(near[0][0, 0], last)
    one = g.map_displacements(np.array([2.0 * total, 0.0, -total, 3.0 * total]), 0.5 * total)
    assert np.array_equal(bits(one[[0, 1, 3]]), bits(np.broadcast_to(last, (3, 2))))


@pytest.mark.parametrize("T", gc.REFLECT_TS)
def test_reflecting_restatement_against_the_exact_oracle(T):
    worst = 0.0
    for t, total, scale, disp, s0 in gc.reflect_cases():
        if t != T:
            continue
        g = geo.Geometry([geo.Edge((0.0, 0.0), (total, 0.0))])
        assert g.total_length == total
        _, arc, _ = geo.map_displacements(disp[None], s0, g, boundary="reflect", return_arc_edge=True)
        err, bound = gc.reflect_error(arc[0], disp, s0, total), gc.reflect_bound(T, disp, total)
        worst = max(worst, err / bound)
        print(f"T {T} total {total} scale {scale}: error {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (T, total, scale)
        assert (arc >= 0).all() and (arc <= total).all()
    print(f"T {T}: worst error / bound {worst:.3g}")


def test_reflecting_walk_keeps_the_uniform_law():
    """8192 uniform starts, 64 steps of sigma 0.3 total: the uniform law on [0, total] is stationary under reflection, so the
    final mean is total / 2 with sigma total / sqrt(12 * 8192); bound 6 sigma"""
    n, total = 8192, 1550.0
    rng = np.random.default_rng(77)
    g = _geom("serpentine")
    _, arc, _ = geo.map_displacements(rng.standard_normal((n, 64)) * 0.3 * total, rng.uniform(0, total, n), g,
                                      boundary="reflect", return_arc_edge=True)
    sigma = total / np.sqrt(12 * n)
    gap = abs(arc[:, -1].mean() - total / 2) / sigma
    print(f"mean of the final arc: {gap:.2f} sigma from total / 2, variance ratio {arc[:, -1].var() / (total ** 2 / 12):.4f}")
    assert gap <= 6.0


def test_non_finite_steps_stay_on_the_geometry():
    g = _geom("pythagorean")
    total = g.total_length
    disp = np.array([[1.0, np.nan, 5.0, np.inf, -3.0, -np.inf, 2.0, np.nan]])
    for boundary in geo.BOUNDARIES:
        pos, arc, edge = geo.map_displacements(disp, [20.0], g, boundary=boundary, return_arc_edge=True)
        assert (edge >= 0).all() and (edge < len(g.edges)).all()
        assert np.isfinite(pos).all() and np.isfinite(arc).all() and (arc >= 0).all() and (arc <= total).all()
        if boundary == "clamp":
            assert arc[0].tolist() == [21.0, 0.0, 5.0, total, total - 3.0, 0.0, 2.0, 0.0]
    _, arc, _ = geo.map_displacements(np.zeros((3, 1)), [np.nan, np.inf, -np.inf], g, return_arc_edge=True)
    assert arc[:, 0].tolist() == [0.0, total, 0.0]


def test_every_value_error():
    E, G = geo.Edge, geo.Geometry
    with pytest.raises(ValueError, match="Edges don't connect properly at index 0"):
        G([E((0, 0), (1, 0)), E((1, 1), (2, 1))])
    with pytest.raises(ValueError, match="zero length"):
        G([E((0, 0), (1, 0)), E((1, 0), (1, 0))])
    with pytest.raises(ValueError, match="non-finite"):
        G([E((0, 0), (np.inf, 0))])
    with pytest.raises(ValueError, match="empty"):
        G([])
    with pytest.raises(ValueError, match="empty"):
        geo.pack_geometries([[]])
    G([E((0, 0), (1, 0)), E((1 + 1e-12, 0), (2, 1))])                      # np.allclose, as in the reference
    g = _geom("single")
    with pytest.raises(ValueError, match="boundary"):
        g.map_displacements(np.zeros(3), boundary="absorb")
    with pytest.raises(ValueError, match="one start per particle"):
        g.map_displacements(np.zeros((3, 4)), [0.0, 1.0])
    with pytest.raises(ValueError, match="geom_of"):
        geo.map_displacements(np.zeros((2, 4)), 0.0, [g, g], [0, 2])
    with pytest.raises(ValueError, match="geom_of"):
        geo.map_displacements(np.zeros((2, 4)), 0.0, [g, g], [0.0, 1.0])
    with pytest.raises(ValueError, match=r"\[N, T\]"):
        geo.map_displacements(np.zeros((2, 4, 1)), 0.0, g)
    with pytest.raises(ValueError):
        geo.cristae_geometry(0, 1, 1, 1)
    with pytest.raises(ValueError):
        geo.cristae_geometry(2, 1, 0.0, 1)


def test_packed_arrays():
    geoms = [_geom("pythagorean"), _geom("single")]
    p = geo.pack_geometries(geoms)
    assert p["verts"].shape == (6, 2) and p["vert_offsets"].tolist() == [0, 4, 6] and p["vert_offsets"].dtype == np.int32
    assert p["lengths"].tolist() == [50.0, 60.0, 80.0, 0.0, 13.0, 0.0] and p["totals"].tolist() == [190.0, 13.0]
    assert np.array_equal(p["verts"][:4], np.array(gc.GOLDEN_POINTS["pythagorean"], dtype=np.float64))


def test_disp_fbm_scaling_and_exponent_one():
    T, D, dt = 300, 0.7, 0.25
    z = torch.randn(1, T, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    got = geo.disp_fbm(1.0, D, T, dt, generator=torch.Generator().manual_seed(4))
    assert isinstance(got, np.ndarray) and got.shape == (T,) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits((z * np.sqrt(2 * D * dt)).reshape(T).numpy()))
    half = geo.disp_fbm(0.5, D, T, dt, generator=torch.Generator().manual_seed(4))
    unit = gen.fractional_gaussian_noise(z, 0.5).reshape(T).numpy()
    assert np.array_equal(bits(half), bits(unit * np.sqrt(2 * D * dt))) and not np.array_equal(half, got)
    # unit scaling: every displacement has <x^2> = 2 D deltaT.  Mean of 2048 squares: the variance of the mean of n correlated
    # chi^2_1 terms is (2 / n) (1 + 2 sum_k gamma_k^2) <= 2.5 / n at alpha = 0.5 (gamma_1 = -0.29, the rest below 0.06); 6 sigma
    long = geo.disp_fbm(0.5, D, 2048, dt, generator=torch.Generator().manual_seed(9))
    assert abs((long ** 2).mean() / (2 * D * dt) - 1) <= 6 * np.sqrt(2.5 / 2048)
    # and it drives a geometry as in the reference's notebook
    pos = _geom("serpentine").map_displacements(geo.disp_fbm(0.5, 50.0, 200, generator=torch.Generator().manual_seed(1)), 700.0)
    assert pos.shape == (200, 2)


def test_cristae_geometry():
    g = geo.cristae_geometry(3, 8.0, 10.0, 4.0, lead=5.0, origin=(2.0, 1.0))
    assert len(g.edges) == 3 * 3 + 2 + 2 and g.total_length == 3 * 24.0 + 2 * 8.0 + 2 * 5.0
    assert tuple(g.edges[0].start_point) == (2.0, 1.0) and tuple(g.edges[-1].end_point) == (2.0 + 10.0 + 12.0 + 16.0, 1.0)
    assert (g.min_y, g.max_y) == (1.0, 11.0)
    g = geo.cristae_geometry(2, 100.0, (200.0, 250.0), 30.0)
    assert len(g.edges) == 7 and g.total_length == 2 * 30.0 + 400.0 + 500.0 + 100.0
    want = [(0, 0), (0, 200), (30, 200), (30, 0), (130, 0), (130, 250), (160, 250), (160, 0)]
    assert np.array_equal(geo.pack_geometries(g)["verts"], np.array(want, dtype=np.float64))
    assert len(geo.cristae_geometry(1, 1.0, 1.0, 1.0).edges) == 3
    # the ten-edge example of the reference's notebook: an entry edge, a lead, two fingers of different depth, a shorter tail
    g = geo.cristae_geometry(2, 100, (200, 250), 30, lead=100, entry=300, tail=90)
    assert np.array_equal(geo.pack_geometries(g)["verts"], np.array(gc.GOLDEN_POINTS["serpentine"], dtype=np.float64))
    assert len(g.edges) == 10 and g.total_length == 1550.0
    assert [e.color for e in g.edges] == ["blue", "blue", "cyan", "cyan", "cyan", "blue", "cyan", "cyan", "cyan", "blue"]
    assert len(geo.cristae_geometry(1, 1.0, 1.0, 1.0, lead=2.0, tail=0.0).edges) == 4


PROPS, OLD_KEYS, movie_geometries, check_movie = gc.PROPS, gc.OLD_KEYS, gc.movie_geometries, gc.check_movie


@pytest.mark.parametrize("boundary", geo.BOUNDARIES)
@pytest.mark.parametrize("alphas", [None, 0.5])
def test_simulate_movie_on_geometries(alphas, boundary):
    geoms = movie_geometries()
    movie, truth = gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, image_props=PROPS, generator=torch.Generator().manual_seed(8),
                                      device="cpu", alphas=alphas, geometry=geoms, boundary=boundary)
    check_movie(movie, truth, geoms, alphas, "cpu")
    again = gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, image_props=PROPS, generator=torch.Generator().manual_seed(8),
                               device="cpu", alphas=alphas, geometry=geoms, boundary=boundary)
    assert torch.equal(movie, again[0]) and torch.equal(truth["arc"], again[1]["arc"])
    # a single Geometry and an explicit assignment
    _, t1 = gen.simulate_movie(5, 6, 40, 48, 0.4, 4, image_props=PROPS, generator=torch.Generator().manual_seed(8),
                               geometry=geoms[1], boundary=boundary)
    assert t1["geometry_id"].tolist() == [0] * 5
    _, t2 = gen.simulate_movie(5, 6, 40, 48, 0.4, 4, image_props=PROPS, generator=torch.Generator().manual_seed(8),
                               geometry=geoms, geometry_of=[1, 1, 0, 1, 0], boundary=boundary)
    assert t2["geometry_id"].tolist() == [1, 1, 0, 1, 0]


@pytest.mark.parametrize("boundary", geo.BOUNDARIES)
@pytest.mark.parametrize("alpha", [None, 0.5])
def test_simulate_movie_walks_as_specified(alpha, boundary):
    """the draws repeated with the same seed: rand(Np) times the total is the start arc, then z = randn(Np, T, 1), steps
    z * sqrt(2 D / npos) (the fractional noise and its rescale with alphas), steps[:, 0] = 0, then map_displacements"""
    Np, F, npos, D = 5, 6, 4, 0.4
    T = F * npos
    geoms = movie_geometries()
    _, truth = gen.simulate_movie(Np, F, 40, 48, D, npos, image_props=PROPS, generator=torch.Generator().manual_seed(21),
                                  device="cpu", alphas=alpha, geometry=geoms, boundary=boundary)
    g = torch.Generator().manual_seed(21)
    geom_id = np.arange(Np) % 2
    totals = np.array([x.total_length for x in geoms])[geom_id]
    start = torch.rand(Np, generator=g).double().numpy() * totals
    z = torch.randn(Np, T, 1, generator=g)
    Dv = torch.full((Np,), D, dtype=torch.float64)
    if alpha is None:
        steps = z * torch.sqrt(2.0 * Dv.float() / npos).view(Np, 1, 1)
    else:
        rescale = torch.from_numpy(np.power(float(npos), 1.0 - np.full(Np, alpha))).float()
        steps = gen.fractional_gaussian_noise(z.double(), alpha).float() * torch.sqrt(2.0 * Dv.float() / npos * rescale).view(Np, 1, 1)
    steps[:, 0] = 0.0
    packed = geo.pack_geometries(geoms)
    packed["verts"] = np.ascontiguousarray(packed["verts"][:, ::-1])                 # the movie's positions are (y, x)
    pos, arc, edge = geo.map_displacements(steps.view(Np, T).double().numpy(), start, packed, geom_id, boundary, True)
    assert np.array_equal(bits(truth["arc"].numpy()), bits(arc)) and np.array_equal(truth["edge"].numpy(), edge)
    assert np.array_equal(truth["pos"].numpy(), pos.astype(np.float32))
    assert np.array_equal(bits(truth["arc"][:, 0].numpy()), bits(start))             # the first step is zero
    ds = np.diff(arc, axis=1)
    assert (np.abs(ds) > 0).mean() > 0.9                                             # and the particles do move
    # the step scale: away from the ends ds is the step itself, variance 2 D / npos (/ npos^alpha: see simulate_movie)
    var = 2 * D / npos if alpha is None else 2 * D / npos ** alpha
    d = steps.view(Np, T).double().numpy()[:, 1:]
    free = arc[:, :-1] + d                                                           # where no end was met (or reflected at)
    inner = (free > 0) & (free < totals[:, None])
    assert inner.sum() > 100
    assert np.allclose(ds[inner], d[inner], rtol=0, atol=1e-12)
    # the mean of n chi^2_1 terms has relative sigma sqrt(2 / n) (a little more with correlation); bound 6 sigma
    assert abs((ds[inner] ** 2).mean() / var - 1) <= 6 * np.sqrt(2.5 / inner.sum())


def test_simulate_movie_without_a_geometry_is_unchanged_and_bad_arguments_raise():
    kw = dict(image_props=PROPS, device="cpu")
    _, truth = gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, generator=torch.Generator().manual_seed(8), **kw)
    assert set(truth) == OLD_KEYS
    _, again = gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, generator=torch.Generator().manual_seed(8), geometry=None,
                                  geometry_of=None, boundary="clamp", **kw)
    assert all(torch.equal(truth[k], again[k]) for k in truth)
    geoms = movie_geometries()
    with pytest.raises(ValueError, match="need a geometry"):
        gen.simulate_movie(5, 6, 40, 48, 0.4, 4, geometry_of=[0] * 5, **kw)
    with pytest.raises(ValueError, match="need a geometry"):
        gen.simulate_movie(5, 6, 40, 48, 0.4, 4, boundary="reflect", **kw)
    with pytest.raises(ValueError, match="boundary"):
        gen.simulate_movie(5, 6, 40, 48, 0.4, 4, geometry=geoms, boundary="absorb", **kw)
    with pytest.raises(ValueError, match="geometry_of"):
        gen.simulate_movie(5, 6, 40, 48, 0.4, 4, geometry=geoms, geometry_of=[0, 1, 2, 0, 1], **kw)
    with pytest.raises(ValueError, match="geometry_of"):
        gen.simulate_movie(5, 6, 40, 48, 0.4, 4, geometry=geoms, geometry_of=[0, 1], **kw)
    outside = geo.cristae_geometry(1, 1.0, 12.0, 10.0, lead=3.0, origin=(8.0, 14.0))           # x = 8 < margin 9
    with pytest.raises(ValueError, match=r"geometry 1: vertex 0 at \(x, y\) = \(8.0, 14.0\)"):
        gen.simulate_movie(5, 6, 40, 48, 0.4, 4, geometry=[geoms[0], outside], **kw)
    high = geo.cristae_geometry(1, 1.0, 20.0, 10.0, origin=(12.0, 14.0))                       # y = 34 > 39 - 9
    with pytest.raises(ValueError, match="vertex 1"):
        gen.simulate_movie(5, 6, 40, 48, 0.4, 4, geometry=high, **kw)
