"""GPU: the kernel of csrc/confine.hip (ops.map_displacements, mivit_map_displacements) BITWISE against the numpy restatement
(helpers/geometry._map_host) in both modes, in clamp mode bitwise against what the real reference returned
(tests/golden/geometry/map.npz), in reflect mode against the exact per-step oracle within the bound of
tests/geometry_common.py.  The shapes are the smallest that reach each branch: T around a wave (64), a pass of the 256 threads
and the LDS chunk (GEOM_CHUNK_T, and more than two chunks), 1 / 2 / 13 / GEOM_MAX_EDGES edges, one workgroup and several,
three geometries with an unsorted assignment, starts outside the range, steps larger than the total."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import geometry_common as gc
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import geometry as geo

pytestmark = pytest.mark.gpu

C = ops.GEOM_CHUNK_T
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def kernel(disp, s0, geoms, geom_of, boundary):
    out = geo.map_displacements(torch.from_numpy(np.array(disp, dtype=np.float64)).cuda(), s0, geoms, geom_of, boundary, True)
    assert all(o.is_cuda for o in out)
    pos, arc, edge = (o.cpu().numpy() for o in out)
    assert pos.dtype == np.float64 and arc.dtype == np.float64 and edge.dtype == np.int32
    assert pos.shape == disp.shape + (2,) and arc.shape == disp.shape and edge.shape == disp.shape
    return pos, arc, edge


def same(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])), f"{what}: pos"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: arc"
    assert np.array_equal(got[2], want[2]), f"{what}: edge"


@functools.lru_cache(maxsize=None)
def three_geometries():
    return tuple(gc.build(gc.random_geometry(E, seed=E), geo.Edge, geo.Geometry) for E in (13, 1, 2))


@functools.lru_cache(maxsize=None)
def reference(N, T, boundary):
    """the shared case (three geometries, unsorted assignment with repeats) and the restatement's answer, computed once"""
    geoms = three_geometries()
    disp, s0, geom_of = gc.batch(N, T, [g.total_length for g in geoms], seed=1000 + T)
    want = geo.map_displacements(disp, s0, geoms, geom_of, boundary, True)
    for a in (disp, s0, geom_of) + tuple(want):
        a.setflags(write=False)
    return disp, s0, geom_of, want


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("boundary", geo.BOUNDARIES)
def test_kernel_is_the_restatement_bitwise_at_every_length(boundary, T):
    disp, s0, geom_of, want = reference(37, T, boundary)
    assert unsorted_with_repeats(geom_of)
    same(kernel(disp, s0, three_geometries(), geom_of, boundary), want, f"T {T} {boundary}")
    total = np.array([g.total_length for g in three_geometries()])[geom_of]
    assert (np.abs(disp).max(1) > total).any() and (s0 < 0).any() and (s0 > total).any()


def unsorted_with_repeats(geom_of):
    return len(geom_of) < 3 or (not np.array_equal(geom_of, np.sort(geom_of)) and len(np.unique(geom_of)) < len(geom_of))


@pytest.mark.parametrize("N", [1, 37])
@pytest.mark.parametrize("E", [1, 2, 13, ops.GEOM_MAX_EDGES])
def test_kernel_is_the_restatement_bitwise_at_every_edge_count(E, N):
    g = gc.build(gc.random_geometry(E, seed=50 + E), geo.Edge, geo.Geometry)
    assert len(g.edges) == E
    disp, s0, geom_of = gc.batch(N, 65, [g.total_length], seed=E)
    for boundary in geo.BOUNDARIES:
        want = geo.map_displacements(disp, s0, g, geom_of, boundary, True)
        got = kernel(disp, s0, g, geom_of, boundary)
        same(got, want, f"E {E} N {N} {boundary}")
        if N > 1:
            assert got[2].max() == E - 1 and got[2].min() == 0                # both ends of the chain are reached


@pytest.mark.parametrize("n_edges,seed", gc.OPEN_END)
def test_no_edge_found_gives_the_last_vertex_and_the_last_edge_on_the_gpu(n_edges, seed):
    """the branch of tests/test_geometry.py::test_no_edge_found_gives_the_last_vertex_and_the_last_edge, through the kernel"""
    g = gc.build(gc.random_geometry(n_edges, seed), geo.Edge, geo.Geometry)
    total, lens = g.total_length, [e.length for e in g.edges]
    rem = gc.open_end_remainder(lens, total)
    assert rem is not None and rem > lens[-1]
    disp, s0, geom_of = gc.batch(37, 65, [total], seed=n_edges)
    last = np.asarray(g.edges[-1].end_point)
    for boundary in geo.BOUNDARIES:
        got = kernel(disp, s0, g, geom_of, boundary)
        same(got, geo.map_displacements(disp, s0, g, geom_of, boundary, True), f"open end, {n_edges} edges, {boundary}")
        pos, arc, edge = got
        open_ = arc == total
        print(f"{n_edges} edges, {boundary}: {int(open_.sum())} samples find no edge")
        if boundary == "clamp":
            assert open_.sum() > 0
        assert np.array_equal(bits(pos[open_]), bits(np.broadcast_to(last, pos[open_].shape)))
        assert (edge[open_] == n_edges - 1).all()
        near = kernel(np.array([[-1e-3]]), total, g, None, boundary)
        assert near[2][0, 0] == n_edges - 1 and not np.array_equal(near[0][0, 0], last)


def test_kernel_matches_the_reference_bitwise_and_keeps_the_tie_rule():
    golden = dict(np.load(gc.GOLDEN))
    assert int(golden["vertex_landings"]) >= 20
    hits = 0
    for name, points in gc.GOLDEN_POINTS.items():
        g = gc.build(points, geo.Edge, geo.Geometry)
        cases = gc.golden_cases(name, g.total_length)
        batch = [c for c in cases if len(c[1]) == gc.GOLDEN_T]
        pos, _, _ = kernel(np.stack([c[1] for c in batch]), np.array([c[2] for c in batch]), g, None, "clamp")
        for k, (case, _, _) in enumerate(batch):
            assert np.array_equal(bits(pos[k]), bits(golden[f"{name}/{case}/pos"])), (name, case)
        case, disp, s0 = cases[-1]                                            # integer steps from an integer start
        pos, arc, edge = kernel(disp[None], s0, g, None, "clamp")
        assert np.array_equal(bits(pos[0]), bits(golden[f"{name}/int/pos"])), name
        inner = gc.interior_vertex_arcs(points)
        on = np.isin(arc[0], inner)
        hits += int(on.sum())
        assert np.array_equal(edge[0][on], np.searchsorted(inner, arc[0][on]))    # the EARLIER edge wins at a vertex
    assert hits == int(golden["vertex_landings"])


@pytest.mark.parametrize("T", gc.REFLECT_TS)
def test_reflecting_kernel_against_the_exact_oracle(T):
    cases = [c for c in gc.reflect_cases() if c[0] == T]
    geoms = [geo.Geometry([geo.Edge((0.0, 0.0), (total, 0.0))]) for total in gc.REFLECT_TOTALS]
    geom_of = np.array([gc.REFLECT_TOTALS.index(c[1]) for c in cases])
    disp, s0 = np.stack([c[3] for c in cases]), np.array([c[4] for c in cases])
    got = kernel(disp, s0, geoms, geom_of, "reflect")
    worst = 0.0
    for k, (_, total, scale, d, s) in enumerate(cases):
        err, bound = gc.reflect_error(got[1][k], d, s, total), gc.reflect_bound(T, d, total)
        worst = max(worst, err / bound)
        print(f"T {T} total {total} scale {scale}: error {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (T, total, scale)
    print(f"T {T}: worst error / bound {worst:.3g}")
    assert (got[1] >= 0).all() and (got[1] <= np.array(gc.REFLECT_TOTALS)[geom_of][:, None]).all()
    same(got, geo.map_displacements(disp, s0, geoms, geom_of, "reflect", True), f"reflect T {T}")


def test_non_finite_steps_stay_on_the_geometry_on_the_gpu():
    g = gc.build(gc.GOLDEN_POINTS["pythagorean"], geo.Edge, geo.Geometry)
    disp = np.array([[1.0, np.nan, 5.0, np.inf, -3.0, -np.inf, 2.0, np.nan], [0.0] * 8, [0.0] * 8, [0.0] * 8, [-0.0] * 8])
    s0 = np.array([20.0, np.nan, np.inf, -np.inf, -0.0])                  # a start of -0 becomes +0, bit for bit
    for boundary in geo.BOUNDARIES:
        got = kernel(disp, s0, g, None, boundary)
        same(got, geo.map_displacements(disp, s0, g, None, boundary, True), boundary)
        assert (got[2] >= 0).all() and (got[2] < 3).all() and np.isfinite(got[0]).all()
    arc = kernel(disp, s0, g, None, "clamp")[1]
    assert arc[0].tolist() == [21.0, 0.0, 5.0, 190.0, 187.0, 0.0, 2.0, 0.0] and arc[1:, 0].tolist() == [0.0, 190.0, 0.0, 0.0]
    assert not np.signbit(arc[4]).any()


@pytest.mark.parametrize("boundary", geo.BOUNDARIES)
def test_kernel_is_deterministic_and_independent_of_the_batch(boundary):
    from moleculardiffusion_mivit_amd import _native as N
    n, T = 37, 257
    geoms = three_geometries()
    disp, s0, geom_of, want = reference(n, T, boundary)
    first = kernel(disp, s0, geoms, geom_of, boundary)
    same(kernel(disp, s0, geoms, geom_of, boundary), first, "second launch")
    perm = np.random.default_rng(13).permutation(n)
    same(kernel(disp[perm], s0[perm], geoms, geom_of[perm], boundary), [a[perm] for a in first], "permuted batch")
    for i in (0, 17, n - 1):
        same(kernel(disp[i:i + 1], s0[i:i + 1], geoms, geom_of[i:i + 1], boundary), [a[i:i + 1] for a in first], f"particle {i} alone")
    # through the C-ABI into the middle of one allocation: the rows around every output keep their canary
    packed = geo.pack_geometries(geoms)
    dev = {k: torch.from_numpy(v).cuda() for k, v in packed.items()}
    dd, sd, gd = torch.from_numpy(disp.copy()).cuda(), torch.from_numpy(s0.copy()).cuda(), torch.from_numpy(geom_of.astype(np.int32)).cuda()
    canary = -123456.789
    pos = torch.full((n + 2, T, 2), canary, dtype=torch.float64, device="cuda")
    arc = torch.full((n + 2, T), canary, dtype=torch.float64, device="cuda")
    edge = torch.full((n + 2, T), -77, dtype=torch.int32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mode = geo.BOUNDARIES.index(boundary)
    args = (vp(dd), vp(sd), vp(gd), vp(dev["verts"]), vp(dev["lengths"]), vp(dev["vert_offsets"]), vp(dev["totals"]), n, T, 3,
            packed["verts"].shape[0], mode)
    N.check(N.lib.mivit_map_displacements(*args, vp(pos[1:]), vp(arc[1:]), vp(edge[1:]), stream), "mivit_map_displacements")
    p, a, e = pos.cpu().numpy(), arc.cpu().numpy(), edge.cpu().numpy()
    for back, c in ((p, canary), (a, canary), (e, -77)):
        assert bool((back[0] == c).all()) and bool((back[-1] == c).all())
    same((p[1:-1], a[1:-1], e[1:-1]), first, "C-ABI")
    # null arc and edge are accepted
    pos2 = torch.full((n + 2, T, 2), canary, dtype=torch.float64, device="cuda")
    N.check(N.lib.mivit_map_displacements(*args, vp(pos2[1:]), None, None, stream), "mivit_map_displacements")
    assert torch.equal(pos2, pos)
    # the inputs are not written
    assert np.array_equal(bits(dd.cpu().numpy()), bits(disp)) and np.array_equal(bits(sd.cpu().numpy()), bits(s0))
    assert np.array_equal(gd.cpu().numpy(), geom_of)
    for k, v in packed.items():
        assert np.array_equal(dev[k].cpu().numpy(), v), k
    same(first, want, "restatement")


def test_empty_inputs_do_not_launch():
    g = three_geometries()[0]
    for shape in ((0, 300), (5, 0), (0, 0)):
        out = geo.map_displacements(torch.zeros(shape, dtype=torch.float64, device="cuda"), 0.0, g, return_arc_edge=True)
        assert all(o.is_cuda for o in out)
        assert tuple(out[0].shape) == shape + (2,) and tuple(out[1].shape) == shape and tuple(out[2].shape) == shape
    torch.cuda.synchronize()


def test_too_many_edges_and_bad_arguments_are_errors_not_launches():
    from moleculardiffusion_mivit_amd import _native as N
    E = ops.GEOM_MAX_EDGES + 1
    g = gc.build(gc.random_geometry(E, seed=3), geo.Edge, geo.Geometry)
    small = three_geometries()[1]
    disp = torch.zeros(2, 8, dtype=torch.float64, device="cuda")
    assert geo.map_displacements(disp.cpu(), 0.0, [small, g]).shape == (2, 8, 2)          # the restatement has no limit
    with pytest.raises(ValueError, match=f"{E} edges.*{ops.GEOM_MAX_EDGES}"):
        geo.map_displacements(disp, 0.0, [small, g])
    packed = geo.pack_geometries(g)
    dev = {k: torch.from_numpy(v).cuda() for k, v in packed.items()}
    s0, gof = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    canary = -5.0
    pos = torch.full((2, 8, 2), canary, dtype=torch.float64, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n, T, G, V, mode, out=pos):
        return N.lib.mivit_map_displacements(vp(disp), vp(s0), vp(gof), vp(dev["verts"]), vp(dev["lengths"]), vp(dev["vert_offsets"]),
                                             vp(dev["totals"]), n, T, G, V, mode, None if out is None else vp(out), None, None, stream)

    assert call(2, 8, 1, E + 1, 0) != 0 and f"more than {ops.GEOM_MAX_EDGES} edges" in N.last_error()
    assert call(2, 8, 1, E + 1, 2) != 0 and "mode" in N.last_error()
    assert call(2, 8, 0, E + 1, 0) != 0 and call(2, 8, 1, 1, 0) != 0 and call(-1, 8, 1, E, 0) != 0
    assert call(2, 8, 1, E, 0, out=None) != 0 and "null" in N.last_error()
    torch.cuda.synchronize()
    assert bool((pos == canary).all())
    dev = {k: torch.from_numpy(v).cuda() for k, v in geo.pack_geometries(small).items()}
    args = (disp, s0, gof, dev["verts"], dev["lengths"], dev["vert_offsets"], dev["totals"])
    assert ops.map_displacements(*args, 0)[0].shape == (2, 8, 2)
    with pytest.raises(ValueError, match="mode"):
        ops.map_displacements(*args, "absorb")
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.map_displacements(disp.cpu(), *args[1:], "clamp")
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.map_displacements(disp.float(), *args[1:], "clamp")
    with pytest.raises(ValueError, match="geom_of"):
        ops.map_displacements(disp, s0, gof + 1, *args[3:], "clamp")
    with pytest.raises(ValueError, match="vert_offsets"):
        ops.map_displacements(disp, s0, gof, dev["verts"], dev["lengths"], dev["vert_offsets"] + 1, dev["totals"], "clamp")


@pytest.mark.parametrize("boundary", geo.BOUNDARIES)
@pytest.mark.parametrize("alphas", [None, 0.5])
def test_simulate_movie_on_geometries_on_the_gpu(alphas, boundary):
    geoms = gc.movie_geometries()
    movie, truth = gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, image_props=gc.PROPS, device="cuda", alphas=alphas,
                                      generator=torch.Generator(device="cuda").manual_seed(8), geometry=geoms, boundary=boundary)
    gc.check_movie(movie, truth, geoms, alphas, "cuda")
    # identical steps: the CUDA and the CPU mapping are bitwise equal
    steps = (torch.randn(5, 24, generator=torch.Generator().manual_seed(2)) * 0.45).double()
    s0 = torch.tensor([0.0, 3.0, 50.0, 7.5, -1.0], dtype=torch.float64)
    on_gpu = geo.map_displacements(steps.cuda(), s0, geoms, None, boundary, True)
    on_cpu = geo.map_displacements(steps, s0, geoms, None, boundary, True)
    same([o.cpu().numpy() for o in on_gpu], [o.numpy() for o in on_cpu], "simulate_movie's mapping")


def test_simulate_movie_without_a_geometry_is_unchanged_on_the_gpu():
    g = lambda: torch.Generator(device="cuda").manual_seed(8)      # noqa: E731
    _, truth = gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, image_props=gc.PROPS, device="cuda", generator=g())
    assert set(truth) == gc.OLD_KEYS
    _, again = gen.simulate_movie(5, 6, 40, 48, (0.4, 0.01), 4, image_props=gc.PROPS, device="cuda", generator=g(),
                                  geometry=None, geometry_of=None, boundary="clamp")
    assert all(torch.equal(truth[k], again[k]) for k in truth)
