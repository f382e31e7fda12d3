"""GPU: the generating side of the pipeline (fbm.hip, confine.hip, movie.hip, render.hip, deconv.hip) and the two-emitter fit
with its neighbour search (localize2.hip) at the C-ABI, inside the guarded, poisoned buffers of tests/abi_guard.py, through the
harness of tests/abi_call.py: what tests/test_analysis_abi_gpu.py does for the movie-analysis entries.  The numerical suites of
these kernels go through ops.py and helpers/, which reject an out-of-range index before the kernel sees it and allocate
through torch; here every argument is a Buf of exactly the documented size and a C caller's indices reach the kernel, so the
clamps of fgn_kernel, map_displacements_kernel and nb_kernel and the `k < 2 || two` guard of m2_patch run under test.

Per entry: placement (every output written everywhere, the host restatement's value under the bar of the entry's own suite,
imported; one case with every buffer one element off the 256-byte boundary), what the header calls unread filled with
poison (bitwise no difference), the previous contents of the outputs (0x00 against 0xFF: bitwise one result), and the
documented clamps with hostile values that abi_guard.bounded keeps within the guards, against the restatement on the input
sanitised on the host as the header sentence says.  Values that the kernels only compare and never index with (the count of
mivit_fit_spots_mle2, first / last of mivit_render_movie) go to their extremes as they are: no access depends on them.

That these tests can fail was checked on scratch copies of the sources (never committed), each mutation in a library of its
own; what failed, and with which message:
  (a) fgn_kernel without the gamma_row clamp: test_fgn_hostile_gamma_row, C = 1 and 3 ("out: 192 / 576 entries the header
      says are written still hold the fill pattern": the guard's NaN, read as gamma, came through the recursion with the
      poison's own bits); every other fgn test passes, as it should.
  (b) map_displacements_kernel without the geom_of clamp: test_map_displacements_hostile_geom_of at T = 1 reflect and T = 65 in
      both modes ("pos: 6 / 154 / 390 entries differ"); T = 1 clamp passes (the three particles happen to land alike).
  (c) the same kernel without the `v1 > V` clamp: test_map_displacements_hostile_vert_offsets[ends] in clamp mode, T = 1 and 65
      ("pos: 2 / 64 entries ... still hold the fill pattern": where the 13-edge chain finds no edge the walk goes on into the
      guard's lengths and returns the guard's vertex); in reflect mode no sample ends on the total, and [reversed] has no
      offset above V: both pass.
  (d) nb_kernel without `b > n`: test_spot_neighbours_hostile_ends at n = 1, 255, 256 and 257 ("neighbour: 1 entries differ,
      first at [[n - 1]]": the row at (0, 0) found the guard's (-1, -1)).
  (e) m2_patch checking all four guesses whatever the count is: test_fit_spots_mle2_reads_no_second_guess_of_a_single_emitter,
      both tables ("params differs between the two runs").
  (f) m2_patch storing a ninth parameter: every fit_spots_mle2 test that goes through Call, all eleven ("a guard of the
      output params changed").
  (g) ml2_kernel without the stride loop: test_fit_spots_mle2_grid_stride_past_2_to_the_20_workgroups ("params: 1 blocks of 65
      rows differ, first at row 1048515": the block that holds row 2^20); the other eleven pass.
None was left out: every stray access of (a) to (g) stays within the guards of the test's own allocation (at most 1560
bytes beside gamma, 32 beside verts, 24 beside totals, 8 beside ys / xs and params)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import abi_guard as G
import denoise_common as dc
import fbm_common as fc
import geometry_common as gc
import localize2_common as L2
import movie_common as mc
import render_common as rc
import tracking_common as tc
from abi_call import F32, F64, I32, POISON64, Call, bits_equal, check_all, expect, same_results
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import geometry as geo
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
FILLS = ("zero", "poison")                                                # what an output held before the call: 0x00, 0xFF


def both_fills(call, fills=FILLS):
    """the call with its outputs pre-filled with 0x00 and with 0xFF: bitwise one result -> the second call"""
    first, second = (call(out_fill=f) for f in fills)
    same_results(first, second)
    return second


# ----------------------------------------------------------------------------------------------------------------------
# mivit_fgn
# ----------------------------------------------------------------------------------------------------------------------
FGN_T, FGN_U, FGN_N = 65, 3, 5                                            # a gamma row is 520 B: bounded allows +-7 rows
FGN_ALPHAS = (0.5, 1.95, 1.5)
FGN_ROWS = (2, 0, 1, 1, 0)


@functools.lru_cache(maxsize=None)
def fgn_inputs(C):
    z = fc.gaussian(FGN_N, FGN_T, C, seed=40 + C)
    gamma = gen.fgn_autocovariance(FGN_ALPHAS, FGN_T)
    for a in (z, gamma):
        a.setflags(write=False)
    return z, gamma


def fgn_call(z, gamma, rows, mis=0, out_fill=None):
    c = Call("mivit_fgn", mis)
    n, t, C = z.shape
    c.run(c.inp("z", z, F64), c.inp("gamma", gamma, F64), c.inp("gamma_row", rows, I32), n, t, C, len(gamma),
          c.out("out", (n, t, C), F64, out_fill))
    return c


def fgn_close(got, want, what):
    """fbm_common.GAUSS_ATOL, as tests/test_fbm_gpu.py holds the kernel to the restatement and to the Cholesky oracle"""
    worst = float(np.abs(got - want).max())
    print(f"{what}: worst difference {worst:.3e}")
    assert worst <= fc.GAUSS_ATOL, (what, worst)


def fgn_check(c, z, gamma, rows):
    """out against the restatement and against the oracle by definition, on the rows clamped as the header says"""
    rows = np.clip(np.asarray(rows, np.int64), 0, len(gamma) - 1)
    expect(c, "out", gen._fgn_host(z, gamma[rows]), close=fgn_close)
    expect(c, "out", fc.oracle(z, np.asarray(FGN_ALPHAS)[rows]), close=fgn_close)


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("C", [1, 3])
def test_fgn_placement_and_previous_contents(C, mis):
    z, gamma = fgn_inputs(C)
    rows = G.bounded(FGN_ROWS, 0, FGN_U - 1, 8 * FGN_T)
    fgn_check(fgn_call(z, gamma, rows, mis), z, gamma, rows)
    fgn_check(both_fills(lambda out_fill: fgn_call(z, gamma, rows, mis, out_fill)), z, gamma, rows)


@pytest.mark.parametrize("C", [1, 3])
def test_fgn_reads_no_row_of_gamma_that_no_trajectory_names(C):
    z, gamma = fgn_inputs(C)
    rows = G.bounded([2, 0, 2, 2, 0], 0, FGN_U - 1, 8 * FGN_T)
    unread = gamma.copy()
    unread[1] = POISON64
    a = fgn_call(z, unread, rows)
    same_results(a, fgn_call(z, gamma, rows))
    fgn_check(a, z, gamma, rows)


@pytest.mark.parametrize("C", [1, 3])
def test_fgn_hostile_gamma_row(C):
    z, gamma = fgn_inputs(C)
    raw = G.bounded([-3, 0, FGN_U + 2, 1, -1], 0, FGN_U - 1, 8 * FGN_T)
    c = fgn_call(z, gamma, raw)
    clean = fgn_call(z, gamma, np.clip(raw, 0, FGN_U - 1))
    expect(c, "out", clean.outs["out"].numpy())                           # bitwise the clipped call, nothing poisoned
    fgn_check(c, z, gamma, raw)


@pytest.mark.parametrize("C", [1, 3])
def test_fgn_nan_noise_and_an_indefinite_row_stay_on_their_trajectory(C):
    z, gamma = fgn_inputs(C)
    bad_gamma = np.concatenate([gamma, np.zeros((1, FGN_T))])
    bad_gamma[3, :2] = (1.0, 2.0)                                         # kappa = 2 at step 1: v = 1 - 4 goes negative
    rows = np.array(FGN_ROWS)
    clean = fgn_call(z, bad_gamma, G.bounded(rows, 0, FGN_U, 8 * FGN_T))
    bad_z, bad_rows = z.copy(), rows.copy()
    bad_z[1, 10, 0] = np.nan
    bad_rows[3] = 3
    c = fgn_call(bad_z, bad_gamma, G.bounded(bad_rows, 0, FGN_U, 8 * FGN_T))
    got, want = c.outs["out"].numpy(), clean.outs["out"].numpy()
    assert not c.outs["out"].unchanged().numpy().any()
    keep = np.array([k not in (1, 3) for k in range(FGN_N)])
    assert np.isfinite(got[keep]).all() and bits_equal(got[keep], want[keep])
    assert not np.isfinite(got[1]).all() and not np.isfinite(got[3]).all()
    assert np.isnan(got[3, 1:]).all() and np.isfinite(got[1, :10]).all() and np.isfinite(got[1, :, 1:]).all()


# ----------------------------------------------------------------------------------------------------------------------
# mivit_map_displacements
# ----------------------------------------------------------------------------------------------------------------------
GEOM_EDGES_SEEDS = ((1, 1), (2, 3), (13, 0))                              # (edges, seed); the last two are gc.OPEN_END chains
GEOM_N = 7
GEOM_OUTS = ("pos", "arc", "edge")


@functools.lru_cache(maxsize=None)
def geom_packed():
    """(verts [19, 2], lengths [19], vert_offsets [4], totals [3]) of the three polylines, read-only"""
    geoms = [gc.build(gc.random_geometry(E, seed), geo.Edge, geo.Geometry) for E, seed in GEOM_EDGES_SEEDS]
    p = geo.pack_geometries(geoms)
    out = tuple(np.array(p[k]) for k in ("verts", "lengths", "vert_offsets", "totals"))
    assert out[2].tolist() == [0, 2, 5, 19]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def geom_batch(T):
    disp, s0, gof = gc.batch(GEOM_N, T, geom_packed()[3], seed=2000 + T)
    assert not np.array_equal(gof, np.sort(gof)) and set(gof.tolist()) == {0, 1, 2}
    for a in (disp, s0, gof):
        a.setflags(write=False)
    return disp, s0, gof


def map_call(disp, s0, gof, verts, lengths, vo, totals, mode, mis=0, arc=True, edge=True, out_fill=None):
    c = Call("mivit_map_displacements", mis)
    n, t = disp.shape
    c.run(c.inp("disp", disp, F64), c.inp("s0", s0, F64), c.inp("geom_of", gof, I32), c.inp("verts", verts, F64),
          c.inp("lengths", lengths, F64), c.inp("vert_offsets", vo, I32), c.inp("totals", totals, F64), n, t, len(totals),
          len(verts), mode, c.out("pos", (n, t, 2), F64, out_fill), c.out("arc", (n, t), F64, out_fill) if arc else None,
          c.out("edge", (n, t), I32, out_fill) if edge else None)
    return c


def map_ref(disp, s0, gof, verts, lengths, vo, totals, mode):
    """geom_of and vert_offsets clamped on the host as the header says -- g into [0, G - 1], v0 into [0, V - 2], v1 into
    [v0 + 2, V], at most GEOM_MAX_EDGES edges --, then helpers/geometry._map_host on the polyline that leaves, per geometry"""
    n_geom, V = len(totals), len(verts)
    g_of = np.clip(np.asarray(gof, np.int64), 0, n_geom - 1)
    n, t = disp.shape
    pos, arc, edge = np.empty((n, t, 2)), np.empty((n, t)), np.empty((n, t), np.int32)
    for g in np.unique(g_of):
        v0 = min(max(int(vo[g]), 0), V - 2)
        v1 = min(max(int(vo[g + 1]), v0 + 2), V)
        v1 = min(v1, v0 + 1 + ops.GEOM_MAX_EDGES)
        rows = np.nonzero(g_of == g)[0]
        one = {"verts": verts[v0:v1], "lengths": lengths[v0:v1], "vert_offsets": np.array([0, v1 - v0]), "totals": totals[g:g + 1]}
        pos[rows], arc[rows], edge[rows] = geo._map_host(disp[rows], s0[rows], np.zeros(len(rows), np.int64), one, mode)
    return {"pos": pos, "arc": arc, "edge": edge}


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [1, 65])
def test_map_displacements_placement_null_outputs_and_previous_contents(T, mode, mis):
    args = geom_batch(T) + geom_packed() + (mode,)
    want = map_ref(*args)
    whole = geo._map_host(*geom_batch(T), dict(zip(("verts", "lengths", "vert_offsets", "totals"), geom_packed())), mode)
    assert all(bits_equal(want[k], w) for k, w in zip(GEOM_OUTS, whole))   # the sanitised route is the restatement itself
    if T > 1 and mode == 0:                                               # the "no edge found" branch is among the samples
        gof, totals = geom_batch(T)[2], geom_packed()[3]
        open_ = (want["arc"] == totals[gof][:, None]) & (gof == 2)[:, None]
        assert open_.any() and (want["edge"][open_] == 12).all()
    full = map_call(*args, mis)
    check_all(full, want)
    check_all(both_fills(lambda out_fill: map_call(*args, mis, out_fill=out_fill)), want)
    for arc, edge in ((False, True), (True, False), (False, False)):      # arc / edge NULL: pos is bitwise what it was
        c = map_call(*args, mis, arc=arc, edge=edge)
        assert set(c.outs) == {"pos"} | ({"arc"} if arc else set()) | ({"edge"} if edge else set())
        check_all(c, {k: want[k] for k in c.outs})


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [1, 65])
def test_map_displacements_reads_no_unused_slot_and_no_unused_geometry(T, mode):
    disp, s0, gof = geom_batch(T)
    verts, lengths, vo, totals = geom_packed()
    want = map_ref(disp, s0, gof, verts, lengths, vo, totals, mode)
    # the last lengths slot of every geometry, and all of a fourth geometry (two vertices) that no particle uses
    lengths4 = np.concatenate([lengths, [POISON64, POISON64]])
    lengths4[vo[1:] - 1] = POISON64
    verts4 = np.concatenate([verts, np.full((2, 2), POISON64)])
    vo4 = G.bounded(np.concatenate([vo, [len(verts4)]]), 0, len(verts4), 16)
    totals4 = np.concatenate([totals, [POISON64]])
    check_all(map_call(disp, s0, G.bounded(gof, 0, 3, 8), verts4, lengths4, vo4, totals4, mode), want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [1, 65])
def test_map_displacements_hostile_geom_of(T, mode):
    disp, s0, gof = geom_batch(T)
    packed = geom_packed()
    n_geom = len(packed[3])
    raw = np.array(gof)
    raw[np.flatnonzero(gof == 0)[0]] = -3                                 # counts as 0
    raw[np.flatnonzero(gof == n_geom - 1)[0]] = n_geom + 2                # counts as G - 1
    raw[np.flatnonzero(gof == 1)[0]] = -1
    raw = G.bounded(raw, 0, n_geom - 1, 8)                                # geom_of indexes totals (8 B) and vert_offsets (4 B)
    want = map_ref(disp, s0, raw, *packed, mode)
    assert not np.array_equal(np.clip(raw, 0, n_geom - 1), gof)           # ... which is not the well-formed call's result
    check_all(map_call(disp, s0, raw, *packed, mode), want)


@pytest.mark.parametrize("kind", ["ends", "reversed"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [1, 65])
def test_map_displacements_hostile_vert_offsets(T, mode, kind):
    disp, s0, gof = geom_batch(T)
    verts, lengths, vo, totals = geom_packed()
    V = len(verts)
    raw = np.array(vo, np.int64)
    if kind == "ends":
        raw[0], raw[-1] = -3, V + 2
        lengths = lengths.copy()
        lengths[vo[1:] - 1] = POISON64                                    # still unread: the clamped ranges are the packed ones
    else:
        raw[-2], raw[-1] = raw[-1], raw[-2]                               # 0, 2, 19, 5: geometry 1 runs on through geometry 2
    raw = G.bounded(raw, 0, V, 16)                                        # vert_offsets indexes verts (16 B) and lengths (8 B)
    want = map_ref(disp, s0, gof, verts, lengths, raw, totals, mode)
    sane = map_ref(disp, s0, gof, *geom_packed(), mode)
    if kind == "ends":
        assert all(bits_equal(want[k], sane[k]) for k in GEOM_OUTS)       # bitwise the sane call
    else:
        # geometry 2 is left with its last edge alone (v0 = 19 -> 17, v1 = 5 -> 19), far shorter than its stored total:
        # mostly "no edge found", the last vertex and edge 0 of the polyline the rules leave
        two = gof == 2
        beyond = want["arc"][two] > lengths[V - 2]
        assert beyond.any() and (want["edge"][two] == 0).all()
        assert bits_equal(want["pos"][two][beyond], np.broadcast_to(verts[V - 1], want["pos"][two].shape)[beyond])
        assert not bits_equal(want["pos"], sane["pos"]) and bits_equal(want["pos"][gof == 0], sane["pos"][gof == 0])
    check_all(map_call(disp, s0, gof, verts, lengths, raw, totals, mode), want)


# ----------------------------------------------------------------------------------------------------------------------
# mivit_spot_neighbours
# ----------------------------------------------------------------------------------------------------------------------
NB_SIZES = (1, 255, 256, 257)                                             # the block is 256 threads
NB_F, NB_REACH = 4, 2


@functools.lru_cache(maxsize=None)
def nb_table(n):
    """(frame_offsets [5], frames [n], ys [n], xs [n]): four frames, frame 1 empty, the last row at (0, 0) in the last frame"""
    a = n // 3
    counts = np.array([a, 0, a, n - 2 * a])
    rng = np.random.default_rng(60 + n)
    ys, xs = rng.integers(0, 30, n), rng.integers(0, 30, n)
    ys[-1] = xs[-1] = 0
    out = np.concatenate([[0], np.cumsum(counts)]), np.repeat(np.arange(NB_F), counts), ys, xs
    for arr in out:
        arr.setflags(write=False)
    return out


def nb_call(fo, ys, xs, reach=NB_REACH, mis=0, out_fill=None):
    c = Call("mivit_spot_neighbours", mis)
    n = len(ys)
    c.run(c.inp("frame_offsets", fo, I32), c.inp("ys", ys, I32), c.inp("xs", xs, I32), len(fo) - 1, n, reach,
          c.out("neighbour", n, I32, out_fill), c.out("n_neighbours", n, I32, out_fill))
    return c


def nb_ref(frames, ys, xs, reach=NB_REACH):
    return dict(zip(("neighbour", "n_neighbours"), L2.brute_neighbours(frames, ys, xs, reach)))


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n", NB_SIZES)
def test_spot_neighbours_placement_and_previous_contents(n, mis):
    fo, frames, ys, xs = nb_table(n)
    want = nb_ref(frames, ys, xs)
    assert n < 255 or ((want["neighbour"] == -1).any() and want["n_neighbours"].max() > 2)
    fo = G.bounded(fo, 0, n, 4)
    check_all(nb_call(fo, ys, xs, mis=mis), want)
    # -1 is a legal neighbour, so 0xFF would pass for a written value: 0x00 against the garbage pattern here
    check_all(both_fills(lambda out_fill: nb_call(fo, ys, xs, mis=mis, out_fill=out_fill), ("zero", "garbage")), want)
    host = T._spot_neighbours_numpy(fo, ys, xs, NB_REACH)
    assert np.array_equal(host[0], want["neighbour"]) and np.array_equal(host[1], want["n_neighbours"])


@pytest.mark.parametrize("n", NB_SIZES)
def test_spot_neighbours_hostile_ends(n):
    """a read of the row behind the table would find the int32 guard, (-1, -1): within reach of the last row at (0, 0)"""
    fo, frames, ys, xs = nb_table(n)
    assert fo[0] == 0 and fo[-1] == n and frames[-1] == NB_F - 1 and NB_REACH >= 1
    raw = np.array(fo)
    raw[0], raw[-1] = -3, n + 2
    check_all(nb_call(G.bounded(raw, 0, n, 4), ys, xs), nb_ref(frames, ys, xs))


@pytest.mark.parametrize("end", ["front", "back", "both"])
@pytest.mark.parametrize("n", NB_SIZES)
def test_spot_neighbours_offsets_that_do_not_ascend_are_memory_safe(n, end):
    """the header defines no frames for them: guards and inputs intact (run), every entry written and a row or a count"""
    fo, _, ys, xs = nb_table(n)
    raw = np.array(fo)
    if end in ("front", "both"):
        raw[0] = raw[1] + 2
    if end in ("back", "both"):
        raw[-1] = raw[-2] - 3
    c = nb_call(G.bounded(raw, 0, n, 4), ys, xs)
    nb, cnt = c.outs["neighbour"].numpy(), c.outs["n_neighbours"].numpy()
    assert not c.outs["neighbour"].unchanged().numpy().any() and not c.outs["n_neighbours"].unchanged().numpy().any()
    assert ((nb == -1) | ((nb >= 0) & (nb < n))).all() and ((cnt >= 0) & (cnt < n)).all()


# ----------------------------------------------------------------------------------------------------------------------
# mivit_fit_spots_mle2
# ----------------------------------------------------------------------------------------------------------------------
M2_OUTS = ("params", "crlb", "deviance", "status", "iterations")
M2_SET = 65
M2_GRID = 1 << 20                                                         # M2_MAX_GRID of csrc/localize2.hip


def fit_close(got, want, what):
    """tracking_common.KERNEL_FIT_RTOL relative, as tests/test_localize2_gpu.py measures it; NaN where the restatement has NaN"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want == got, 0.0, np.abs(got - want) / np.abs(want))
    worst = float(np.nanmax(rel)) if rel.size else 0.0
    print(f"{what}: worst relative difference {worst:.3e}")
    assert worst <= tc.KERNEL_FIT_RTOL, (what, worst)


M2_CLOSE = {"params": fit_close, "crlb": fit_close, "deviance": fit_close}


def m2_call(name, patches, count, guess, mis=0, out_fill=None):
    c = Call("mivit_fit_spots_mle2", mis)
    n, P = len(patches), patches.shape[1]
    kw = L2.camera_kwargs(name)
    c.run(c.inp("patches", patches, F32), c.inp("count", count, I32), c.inp("guess", guess, F64), n, P, kw["gain"], kw["offset"],
          kw["read_var"], kw["sigma0"], 1 if kw["fit_sigma"] else 0, T.FIT_XTOL, c.out("params", (n, 8), F64, out_fill),
          c.out("crlb", (n, 8), F64, out_fill), c.out("deviance", n, F64, out_fill), c.out("status", n, I32, out_fill),
          c.out("iterations", n, I32, out_fill))
    return c


def m2_rows(name, n=M2_SET):
    return tuple(a[:n] for a in L2.case_table(name))


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n", [1, M2_SET])
@pytest.mark.parametrize("name", ["p5_fixed", "p15_camera"])
def test_fit_spots_mle2_placement_and_previous_contents(name, n, mis):
    want = dict(zip(M2_OUTS, (a[:n] for a in L2.case_reference(name))))
    check_all(m2_call(name, *m2_rows(name, n), mis), want, close=M2_CLOSE)
    second = both_fills(lambda out_fill: m2_call(name, *m2_rows(name, n), mis, out_fill))
    check_all(second, want, close=M2_CLOSE)
    one = m2_rows(name, n)[1] == 1
    assert np.isnan(second.outs["params"].numpy()[one][:, 3:6]).all() and np.isnan(second.outs["crlb"].numpy()[one][:, 3:6]).all()


@pytest.mark.parametrize("name", ["p5_fixed", "p9"])
def test_fit_spots_mle2_reads_no_second_guess_of_a_single_emitter(name):
    patches, count, guess = m2_rows(name)
    one = count == 1
    assert 0 < one.sum() < M2_SET
    poisoned, zeroed = guess.copy(), guess.copy()
    poisoned[one, 2:] = POISON64
    zeroed[one, 2:] = 0.0
    a = m2_call(name, patches, count, poisoned)
    same_results(a, m2_call(name, patches, count, zeroed))
    assert (a.outs["status"].numpy()[one] != 3).all() and (a.outs["status"].numpy()[one] == 0).any()
    check_all(a, dict(zip(M2_OUTS, (x[:M2_SET] for x in L2.case_reference(name)))), close=M2_CLOSE)


def test_fit_spots_mle2_a_count_that_is_neither_1_nor_2():
    """count is compared with 1 and 2 and indexes nothing, so its extremes go in as they are"""
    name = "p9"
    patches, count, guess = m2_rows(name)
    at = np.array([3, 20, 41, 68])                                        # where the odd rows stand in the longer batch
    odd = np.array([0, 3, -1, INT_MAX])
    n = M2_SET + len(at)
    regular = np.ones(n, bool)
    regular[at] = False
    src = np.zeros(n, np.int64)
    src[regular] = np.arange(M2_SET)
    src[at] = (4, 21, 41, 64)                                             # an odd row carries a regular neighbour's patch and guess
    count2 = np.array(count[src], np.int64)
    count2[at] = odd
    c = m2_call(name, patches[src], count2, guess[src])
    clean = m2_call(name, patches, count, guess)
    want = {k: np.empty(c.outs[k].shape, clean.outs[k].numpy().dtype) for k in M2_OUTS}
    for k in M2_OUTS:
        want[k][regular] = clean.outs[k].numpy()                          # bitwise their result without the odd rows
        want[k][at] = {"status": 3, "iterations": 0}.get(k, np.nan)
    check_all(c, want)


def guarded_on_device(shape, dtype):
    """an output too large to inspect on the host: body of exactly the documented size between two poisoned guards, all of it
    poison -> (raw bytes, body view)"""
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((G.GUARD_BYTES + nbytes + G.GUARD_BYTES,), G.POISON, dtype=torch.uint8, device="cuda")
    body = raw[G.GUARD_BYTES:G.GUARD_BYTES + nbytes]
    assert body.data_ptr() % 8 == 0
    return raw, body.view(dtype).reshape(shape)


def test_fit_spots_mle2_grid_stride_past_2_to_the_20_workgroups():
    """N = 2^20 + 65 patches, the first 65 rows of p5_fixed over and over: more patches than workgroups of a launch, so the
    first 65 workgroups take a second patch.  Every row is bitwise the row of the 65-row call; compared on the device.
    Measured on the MI355X: the launch takes 105 ms, the whole test 0.4 s."""
    name = "p5_fixed"
    patches, count, guess = m2_rows(name)
    small = m2_call(name, patches, count, guess)
    n = M2_GRID + M2_SET
    reps, rest = divmod(n, M2_SET)
    idx = torch.arange(n, device="cuda") % M2_SET
    ins = [torch.from_numpy(np.array(a)).cuda()[idx].contiguous() for a in (patches, count, guess)]
    keep = [t.clone() for t in ins]
    shapes = {"params": ((n, 8), F64), "crlb": ((n, 8), F64), "deviance": ((n,), F64), "status": ((n,), I32), "iterations": ((n,), I32)}
    outs = {k: guarded_on_device(*v) for k, v in shapes.items()}
    kw = L2.camera_kwargs(name)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    N.check(N.lib.mivit_fit_spots_mle2(*(t.data_ptr() for t in ins), n, 5, kw["gain"], kw["offset"], kw["read_var"], kw["sigma0"],
                                       1 if kw["fit_sigma"] else 0, T.FIT_XTOL, *(outs[k][1].data_ptr() for k in M2_OUTS),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mivit_fit_spots_mle2")
    stop.record()
    torch.cuda.synchronize()
    print(f"mivit_fit_spots_mle2, N = {n}, P = 5: {start.elapsed_time(stop):.1f} ms")
    assert all(torch.equal(a, b) for a, b in zip(ins, keep)), "an input was written"
    for k in M2_OUTS:
        raw, body = outs[k]
        assert bool((raw[:G.GUARD_BYTES] == G.POISON).all()) and bool((raw[-G.GUARD_BYTES:] == G.POISON).all()), f"a guard of {k} changed"
        block = small.outs[k].body().cuda()
        bits = (lambda t: t.contiguous().view(torch.int64)) if block.dtype == F64 else (lambda t: t)
        got = bits(body).reshape((n,) + tuple(block.shape[1:]))
        full = got[:reps * M2_SET].reshape((reps, M2_SET) + tuple(block.shape[1:]))
        differ = (full != bits(block)[None]).reshape(reps, -1).any(dim=1)
        assert not bool(differ.any()), f"{k}: {int(differ.sum())} blocks of 65 rows differ, first at row {int(differ.nonzero()[0]) * M2_SET}"
        assert torch.equal(got[reps * M2_SET:], bits(block)[:rest]), f"{k}: the last {rest} rows differ"


# ----------------------------------------------------------------------------------------------------------------------
# mivit_render_movie
# ----------------------------------------------------------------------------------------------------------------------
def smallest(cases, size):
    return min(cases, key=size)["id"]


MOVIE_SMALLEST = smallest(mc.cases(), lambda c: (c["F"] * c["H"] * c["W"], c["amp"].size))


def movie_call(c, first="case", last="case", pos=None, amp=None, mis=0, out_fill=None):
    call = Call("mivit_render_movie", mis)
    first = c["first"] if isinstance(first, str) else first
    last = c["last"] if isinstance(last, str) else last
    pos, amp = (c["pos"] if pos is None else pos), (c["amp"] if amp is None else amp)
    call.run(call.inp("pos", pos, F32), call.inp("amp", amp, F32), None if first is None else call.inp("first", first, I32),
             None if last is None else call.inp("last", last, I32), len(amp), c["F"], c["npos"], c["sigma"], c["up"], c["radius"],
             c["H"], c["W"], call.out("movie", (c["F"], c["H"], c["W"]), F32, out_fill))
    return call


def movie_close(cid):
    """the per-pixel bar of tests/movie_common.py, as tests/test_movie_render_gpu.py applies it, and its outer check"""
    def close(got, want, what):
        err, bar = np.abs(got.astype(np.float64) - want), mc.bar(cid).reshape(-1)
        print(f"{what}: worst error / bar {mc.ratio(got, want, bar)[0]:.3f}")
        assert ((err < bar) | (err == 0)).all() and mc.outer_ok(got, want)[0], what
        assert (got[want == 0] == 0).all(), what
    return close


def expect_close(call, name, want, close):
    """expect with a reference of higher precision than the output: the placement checks, then close(got, want)"""
    expect(call, name, call.outs[name].numpy(), close=lambda got, _, what: close(got, np.asarray(want).reshape(-1), what))


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("cid", [MOVIE_SMALLEST, "lifetimes"])
def test_render_movie_placement_and_previous_contents(cid, mis):
    c, ref = mc.case(cid), mc.table()[cid]["ref"]
    expect_close(movie_call(c, mis=mis), "movie", ref, movie_close(cid))
    expect_close(both_fills(lambda out_fill: movie_call(c, mis=mis, out_fill=out_fill)), "movie", ref, movie_close(cid))


def test_render_movie_first_and_last_at_their_extremes():
    """first / last are compared with the frame and index nothing (movie.hip:74), so INT_MIN and INT_MAX go in as they are"""
    c = mc.case("lifetimes")
    Np = c["Np"]
    null = movie_call(c, first=None, last=None)
    always = movie_call(c, first=np.full(Np, INT_MIN, np.int64), last=np.full(Np, INT_MAX, np.int64))
    same_results(null, always)                                            # visible in every frame: the movie of NULL / NULL
    assert not bits_equal(null.outs["movie"].numpy(), movie_call(c).outs["movie"].numpy())
    for k in (0, 3, Np - 1):                                              # particle k never visible: the movie without it
        first, last = np.full(Np, INT_MIN, np.int64), np.full(Np, INT_MAX, np.int64)
        first[k], last[k] = INT_MAX, INT_MIN
        keep = np.arange(Np) != k
        without = movie_call(c, first=None, last=None, pos=c["pos"][keep], amp=c["amp"][keep])
        assert not bits_equal(without.outs["movie"].numpy(), null.outs["movie"].numpy()), "the particle contributes to this movie"
        same_results(movie_call(c, first=first, last=last), without)


# ----------------------------------------------------------------------------------------------------------------------
# mivit_render_frames
# ----------------------------------------------------------------------------------------------------------------------
FRAMES_SMALLEST = smallest(rc.cases(), lambda c: (c["amp"].shape[0] * len(c["sigmas"]) * c["amp"].shape[1] * c["P"] ** 2, c["amp"].size))


def frames_call(c, mis=0, out_fill=None):
    call = Call("mivit_render_frames", mis)
    n, t, _ = c["traj"].shape
    nsig = len(c["sigmas"])
    call.run(call.inp("traj", c["traj"], F32), n, t, c["npos"], call.inp("sigmas", np.array(c["sigmas"]), F32), nsig, c["P"], c["up"],
             call.inp("amp", c["amp"], F32), int(c["center"]), call.out("out", (n, nsig, t // c["npos"], c["P"], c["P"]), F32, out_fill))
    return call


def frames_close(cid):
    """the per-pixel bar of tests/render_common.py, as tests/test_render_frames_gpu.py applies it, and its outer check"""
    def close(got, want, what):
        err, bar = np.abs(got.astype(np.float64) - want), rc.bar(cid).reshape(-1)
        print(f"{what}: worst error / bar {rc.ratio(got, want, bar)[0]:.3f}")
        assert np.isfinite(got).all() and (err <= bar).all() and rc.outer_ok(got, want)[0], what
    return close


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("cid", [FRAMES_SMALLEST, "nsig2-7x2"])
def test_render_frames_placement_and_previous_contents(cid, mis):
    c, ref = rc.case(cid), rc.table()[cid]["ref"]
    assert np.array(c["sigmas"], np.float32).astype(np.float64).tolist() == c["sigmas"]   # what the kernel reads is what the reference read
    expect_close(frames_call(c, mis), "out", ref, frames_close(cid))
    expect_close(both_fills(lambda out_fill: frames_call(c, mis, out_fill)), "out", ref, frames_close(cid))


# ----------------------------------------------------------------------------------------------------------------------
# mivit_rl_tv_deconvolve, mivit_gaussian_filter_frames: bitwise / to the last bit, as tests/test_denoise_gpu.py
# ----------------------------------------------------------------------------------------------------------------------
def small_psf(K):
    p = np.random.default_rng(100 + K).random((K, K)) + 0.05
    return p / p.sum()


def rl_call(x, psf, its, tvw, mis=0, out_fill=None):
    c = Call("mivit_rl_tv_deconvolve", mis)
    B, S, H, W = x.shape
    arr = (ctypes.c_int * len(its))(*its)                                 # a HOST array
    c.run(c.inp("frames", x, F32), B, S, H, W, c.inp("psf", psf, F64), len(psf), arr, len(its), tvw,
          c.out("out", (B, len(its), S, H, W), F32, out_fill))
    return c


# the smallest entry of the suite's lists (H = 1, K = 1, one snapshot, no TV term), and one with an even PSF and a batch
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("B,S,H,W,K,its,tvw", [(3, 1, 1, 1, 1, (0,), 0.0), (2, 3, 5, 7, 4, (1, 4), 0.05)])
def test_rl_tv_deconvolve_placement_and_previous_contents(B, S, H, W, K, its, tvw, mis):
    rng = np.random.default_rng(70 + H)
    x = (rng.random((B, S, H, W)) * 0.9).astype(np.float32)
    psf = small_psf(K)
    want = np.moveaxis(gen._rl_tv_frames(x, psf, list(its), tvw), 0, 1)   # [B, n_snap, S, H, W]
    expect(rl_call(x, psf, its, tvw, mis), "out", want)
    expect(both_fills(lambda out_fill: rl_call(x, psf, its, tvw, mis, out_fill)), "out", want)


def gauss_call(x, sigma, mis=0, out_fill=None):
    c = Call("mivit_gaussian_filter_frames", mis)
    n, H, W = x.shape
    c.run(c.inp("in", x, F32), n, H, W, sigma, 4.0, c.out("out", (n, H, W), F32, out_fill))
    return c


def gauss_close(got, want, what):
    """denoise_common.GAUSS_FILTER_ULPS: the last float32 bit, as tests/test_denoise_gpu.py"""
    ulps = int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32)).max())
    print(f"{what}: {ulps} ulp")
    assert ulps <= dc.GAUSS_FILTER_ULPS, (what, ulps)


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("sigma", [0.5, 2.0])
def test_gaussian_filter_frames_placement_and_previous_contents(sigma, mis):
    x = np.random.default_rng(6).random((7, 13, 5)).astype(np.float32)    # the suite's smallest frames
    want = gen.gaussian_filter_frames(x, sigma)
    expect(gauss_call(x, sigma, mis), "out", want, close=gauss_close)
    expect(both_fills(lambda out_fill: gauss_call(x, sigma, mis, out_fill)), "out", want, close=gauss_close)
