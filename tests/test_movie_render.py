"""CPU half of the whole-field renderer's suite (tests/movie_common.py; GPU half: tests/test_movie_render_gpu.py): the fp64
reference against the naive full-grid loop, what every group of the case table reaches (by restating the integer arithmetic of
csrc/movie.hip: tile of every pair, survivors per (tile, chunk), which inequality of the cull sits at equality), the measured
constants against the written ones, the yardstick inside its own model, the ring condition, and every planted mutation of the
yardstick caught by the bar the kernel is held to.  Needs neither a GPU nor the native library."""
import math

import numpy as np
import pytest

import movie_common as mc

IDS = [c["id"] for c in mc.cases()]


def group(name):
    return [c for c in mc.cases() if c["group"] == name]


@pytest.mark.parametrize("cid", ["ring-default", "amps-overlap"])
def test_reference_matches_the_naive_full_grid_loop(cid):
    """the bound of tests/test_movie_sim.py::test_restatement_matches_naive_loop_within_the_truncation_bound; every position
    of these two entries lies inside the field, where the naive loop's peak on the bounded grid is the definition's"""
    from test_movie_sim import naive_movie
    c, rec = mc.case(cid), mc.table()[cid]
    assert c["pos"].min() > 0 and c["pos"][..., 0].max() < c["H"] - 1 and c["pos"][..., 1].max() < c["W"] - 1
    naive = naive_movie(c["pos"].astype(np.float64), c["amp"].astype(np.float64), c["sigma"], c["H"], c["W"], c["up"])
    total = float(np.abs(c["amp"]).astype(np.float64).sum())
    bound = total * math.exp(-((c["radius"] - 1) * c["up"]) ** 2 / (2 * c["sigma"] ** 2)) + 1e-12 * total
    err = float(np.abs(rec["ref"] - naive).max())
    print(f"{cid}: reference vs naive loop {err:.3e}, truncation bound {bound:.3e}")
    assert 0 < err <= bound
    # the separable magnitudes are those of the same function: no sign in these two entries, so B is the reference itself
    assert np.abs(rec["B"] - rec["ref"]).max() <= 1e-12 * rec["B"].max()
    assert (rec["W"] >= 0).all() and (rec["A"][rec["B"] > 0] > 0).all()


# ---- what the table reaches ---------------------------------------------------------------------------------------------
REACHES = {
    # group: what its entries reach; each claim is asserted by the test of that group below
    "grid": "six fields (2 x 2 tiles, one row / column in the second tile, one tile exactly, 1 x 1, 1 x 200, 70 x 3) x eight (up, sigma, radius): "
            "radius 0 .. the cap of 64, up 1, even, odd and the cap of 64",
    "npos": "1, 5, 7, 256 sub-positions: the cap, one chunk per particle, and a chunk boundary inside particle 36 of 37 x 7 pairs",
    "chunk": "255, 256, 257, 512, 513 pairs; the last pair alone lights its window",
    "batch": "1, 63, 64, 65, 128, 129, 256 survivors of one chunk in one tile behind culled pairs; a lone survivor in lane 63 of wave 3",
    "cull": "each inequality of the cull at equality and one pixel short of it, at the field's border and at the tile seam, radius 0, 3, 8",
    "ring": "an interior particle whose outermost ring is >= 100 x the bar, at radius 3 and at the default radius",
    "amps": "1e4 beside 1e-2 (disjoint, overlapping), zeros, -0.0, a negative value, inf / NaN amplitudes among finite ones",
    "ties": "c on an integer and on k + 1/2 (k even, odd), uf a half-integer, the peak sample in the neighbouring pixel",
    "nonfinite": "NaN, +-inf, |c| just below and at 2^30, in one coordinate and in both; a NaN sub-position in a visible particle",
    "lifetimes": "first / last before the movie, after it, one frame, all frames, first == last == F - 1",
    "far": "columns up to 2^20 + 69 and around 2^19, and the same scene at the origin",
}


def test_every_group_is_named_and_within_the_limits():
    assert set(REACHES) == set(mc.groups())
    for c in mc.cases():
        tY, tX = mc.tiles(c)
        assert c["Np"] <= 300 and c["F"] <= 3 and (tY * tX <= 8 or c["group"] == "far"), c["id"]


def test_grid_group_reaches_every_field_and_setting():
    cs = group("grid")
    assert {(c["H"], c["W"]) for c in cs} == set(mc.GRID_FIELDS) and len(cs) == len(mc.GRID_FIELDS) * len(mc.GRID_SETTINGS)
    assert {mc.tiles(c) for c in cs} == {(2, 2), (1, 1), (1, 4), (3, 1)}
    assert mc.tiles(mc.case("grid-33x65-u1s0.3r0")) == (2, 2) and mc.tiles(mc.case("grid-32x64-u1s0.3r0")) == (1, 1)
    sets = {(c["up"], c["radius"]) for c in cs}
    assert sets == {(1, 0), (1, 8), (2, 4), (5, 8), (4, 16), (5, 64), (64, 8)}         # (5, 6.5, default) and (5, 1.5, 8) share (5, 8)
    assert {c["sigma"] for c in cs if (c["up"], c["radius"]) == (5, 8)} == {6.5, 1.5}
    assert max(c["radius"] for c in cs) == mc.gen.MOVIE_MAX_RADIUS and max(c["up"] for c in cs) == mc.gen.MOVIE_MAX_UP
    # default radii are the helper's
    assert mc.case("grid-37x70-u1s1.3rd")["radius"] == math.ceil(5 * float(np.float32(1.3))) + 1
    for c in cs:                                                 # every case lights something and every pair is judged somewhere
        assert mc.table()[c["id"]]["B"].max() > 0 and mc.survivors(c)


def test_npos_group_reaches_the_cap_and_a_chunk_boundary_inside_a_particle():
    cs = {c["npos"]: c for c in group("npos")}
    assert set(cs) == {1, 5, 7, 256} and mc.gen.MOVIE_MAX_NPOS == 256 == mc.CHUNK
    c = cs[7]
    assert c["Np"] == 37 and c["Np"] * 7 == 259
    p, s = divmod(mc.CHUNK, 7)
    assert (p, s) == (36, 4)                                     # pair 256, the first of the second pass, is inside particle 36
    assert {k[3] for k in mc.survivors(c)} == {0, 1}             # and both passes have survivors
    c = cs[256]
    assert c["Np"] == 2 and {k[3] for k in mc.survivors(c)} == {0, 1}


def test_chunk_group_reaches_every_pair_count_and_only_the_last_pair_lights_its_pixels():
    cs = group("chunk")
    assert [c["Np"] * c["npos"] for c in cs] == [255, 256, 257, 512, 513] == [p for p, _ in mc.CHUNK_CASES]
    assert {c["npos"] for c in cs} == {1, 2, 3, 5}
    for c in cs:
        pairs = c["Np"] * c["npos"]
        cov, win = mc.coverage(c)
        last = win[(c["Np"] - 1, 0, c["npos"] - 1)]
        assert len(win) == pairs and (cov[0, last[0]:last[1], last[2]:last[3]] == 1).all()
        assert (last[1] - last[0], last[3] - last[2]) == (5, 5) and last[0] < mc.TH <= last[1] and last[2] == mc.TW
        chunks = {k[3] for k in mc.survivors(c)}
        assert chunks == set(range((pairs + mc.CHUNK - 1) // mc.CHUNK))
        # the last pair is alone in the last pass exactly where the count is one past a multiple of the chunk
        assert ((pairs - 1) % mc.CHUNK == 0) == (pairs in (257, 513))
    assert divmod(mc.CHUNK, 3) == (85, 1)                        # 513 = 171 x 3: the second pass starts inside particle 85


def test_batch_group_reaches_every_survivor_count_with_culled_pairs_in_front():
    cs = {c["id"]: c for c in group("batch")}
    for n in mc.BATCH_SURVIVORS:
        c = cs[f"batch-{n}"]
        surv = mc.survivors(c)
        assert c["npos"] == 1 and c["Np"] <= mc.CHUNK
        assert set(surv) <= {(0, 0, 0, 0), (0, 1, 1, 0)}         # one pass; tile (0, 0) and the tile of the culled pairs
        tids = surv[(0, 0, 0, 0)]
        assert len(tids) == n
        assert len(surv.get((0, 1, 1, 0), [])) == c["Np"] - n and not set(tids) & set(surv.get((0, 1, 1, 0), []))
        if n != 256:                                             # survivor index and thread differ for every survivor
            assert all(t != i for i, t in enumerate(tids))
        else:
            assert tids == list(range(256))
        # the last survivor of each batch of 64, and the last of all, light a pixel of their own
        cov, win = mc.coverage(c)
        cen = mc.centres(c)
        for i in sorted(set(range(mc.BATCH - 1, n, mc.BATCH)) | {n - 1}):
            iy, ix = cen[tids[i], 0, 0]
            assert cov[0, iy, ix] == 1 and win[(tids[i], 0, 0)][0] <= iy < win[(tids[i], 0, 0)][1]
    assert {n // mc.BATCH + (n % mc.BATCH > 0) for n in mc.BATCH_SURVIVORS} == {1, 2, 3, 4}       # 1 .. 4 batches
    surv = mc.survivors(cs["batch-lane255"])
    assert surv[(0, 0, 0, 0)] == [255] and 255 % 64 == 63 and 255 // 64 == 3
    assert len(surv[(0, 1, 1, 0)]) == 255


def test_cull_group_puts_every_inequality_at_equality_and_one_short_of_it():
    cs = group("cull")
    assert {(c["reach"]["at"], c["radius"]) for c in cs} == {(a, r) for a in ("border", "seam") for r in (0, 3, 8)}
    for c in cs:
        cen, r = mc.centres(c), c["radius"]
        tilesY, tilesX = mc.tiles(c)
        assert (tilesY, tilesX) == ((1, 1) if c["reach"]["at"] == "border" else (4, 2))
        cov, win = mc.coverage(c)
        assert cov.max() == 1                                    # disjoint windows: every lit pixel is one particle's alone
        seen = set()
        for p in range(c["Np"]):
            iy, ix = (int(v) for v in cen[p, 0, 0])
            for tY in range(tilesY):
                for tX in range(tilesX):
                    d, holds = mc.margins(iy, ix, r, tY * mc.TH, tX * mc.TW)
                    for k in range(4):
                        if d[k] in (0, -1) and all(holds[j] for j in range(4) if j != k):      # inequality k alone decides
                            seen.add((k, d[k], holds[k], (tY, tX)))
        for k in range(4):
            assert {(kk, dd) for kk, dd, _, _ in seen if kk == k} == {(k, 0), (k, -1)}, (c["id"], k)
        assert all(h == ((d == 0) if k in (0, 2) else (d == -1)) for k, d, h, _ in seen)
        if c["reach"]["at"] == "border":
            # the four particles that hold touch row 0, row H - 1, column 0, column W - 1 with their outermost ring alone
            lit = np.nonzero(cov[0])
            assert set(lit[0]) >= {0, c["H"] - 1} and set(lit[1]) >= {0, c["W"] - 1} and len(win) == 4
            rows = sorted((w[0], w[1]) for w in win.values() if w[1] - w[0] == 1)
            cols = sorted((w[2], w[3]) for w in win.values() if w[3] - w[2] == 1)
            assert (0, 1) in rows and (c["H"] - 1, c["H"]) in rows and (0, 1) in cols and (c["W"] - 1, c["W"]) in cols
        else:
            tiles_seen = {(k, t) for k, _, _, t in seen}
            assert {(0, (1, 0)), (1, (0, 0))} <= tiles_seen       # row 32: first row of tile row 1, one past tile row 0
            assert any(k == 2 and t[1] == 1 for k, t in tiles_seen) and any(k == 3 and t[1] == 0 for k, t in tiles_seen)
            assert len(win) == 8                                  # inside the field every particle is seen by some tile


def test_ring_condition_holds_from_the_reference_alone():
    """the outermost ring of an interior particle is at least 100 x the bar of its pixel, and the ring beyond it is exactly 0
    in the reference: a window one ring short or one ring wide fails the accuracy test"""
    for cid, r in (("ring-r3", 3), ("ring-default", 8)):
        c, rec = mc.case(cid), mc.table()[cid]
        assert c["radius"] == r and c["Np"] == c["F"] == c["npos"] == 1
        iy, ix = (int(v) for v in mc.centres(c)[0, 0, 0])
        assert r + 1 <= iy < c["H"] - r - 1 and r + 1 <= ix < c["W"] - r - 1
        ref, b = rec["ref"][0], mc.bar(cid)[0]
        ring = np.zeros_like(ref, bool)
        ring[iy - r:iy + r + 1, ix - r:ix + r + 1] = True
        ring[iy - r + 1:iy + r, ix - r + 1:ix + r] = False
        worst = float((ref[ring] / b[ring]).min())
        print(f"{cid}: outermost ring / bar >= {worst:.3e}, faintest ring pixel {ref[ring].min():.3e}")
        assert worst >= 100
        beyond = np.zeros_like(ref, bool)
        beyond[iy - r - 1:iy + r + 2, ix - r - 1:ix + r + 2] = True
        beyond[iy - r:iy + r + 1, ix - r:ix + r + 1] = False
        assert (ref[beyond] == 0).all() and (rec["B"][0][beyond] == 0).all()       # there the kernel must give exactly 0


def test_amps_group_reaches_its_amplitudes():
    cs = {c["id"]: c for c in group("amps")}
    for cid, overlap in (("amps-disjoint", False), ("amps-overlap", True)):
        c = cs[cid]
        assert {float(v) for v in c["amp"][:, 0, 0]} == {float(np.float32(1e4)), float(np.float32(1e-2))}
        cov, win = mc.coverage(c)
        both = np.zeros(cov.shape[1:], int)
        for p in (0, 1):
            m = np.zeros_like(both)
            for s in (0, 1):
                w = win[(p, 0, s)]
                m[w[0]:w[1], w[2]:w[3]] = 1
            both += m
        assert (both.max() == 2) == overlap
    a = cs["amps-signs"]["amp"]
    assert ((a == 0) & ~np.signbit(a)).any() and ((a == 0) & np.signbit(a)).any() and (a[1] == 0).all()
    assert (a < 0).sum() == 1 and (a > 0).sum() > 10
    a = cs["amps-nonfinite"]["amp"]
    assert np.isposinf(a).any() and np.isneginf(a).any() and np.isnan(a).any() and np.isfinite(a[4]).all()
    for p in (0, 1, 2):                                          # a non-finite amplitude beside finite ones of the same particle
        assert np.isfinite(a[p]).any() and not np.isfinite(a[p]).all()
    assert np.isfinite(mc.table()["amps-nonfinite"]["ref"]).all()


def test_ties_group_reaches_every_tie():
    cs = group("ties")
    assert {c["up"] for c in cs} == {1, 2, 4, 5}
    pos = np.array(mc.TIE_POSITIONS)
    frac = pos - np.floor(pos)
    assert set(frac.ravel()) == {0.0, 0.5}
    k = np.floor(pos[frac == 0.5]).astype(int)
    assert (k % 2 == 0).any() and (k % 2 == 1).any()             # k + 1/2 for even and odd k: rint goes down and up
    assert (31.5, 63.5) in mc.TIE_POSITIONS and tuple(np.rint([31.5, 63.5])) == (mc.TH, mc.TW)      # the tie decides the tile
    for c in cs:
        up = c["up"]
        cc = c["pos"].reshape(-1)
        ic = np.rint(cc)
        fc = cc - ic
        uf = fc * np.float32(up) + np.float32(0.5) * np.float32(up - 1)
        assert uf.dtype == np.float32 and set(np.abs(fc)) == {0.0, 0.5}
        assert (fc == 0.5).any() and (fc == -0.5).any()
        half = (uf - np.floor(uf)) == 0.5
        g = np.rint(uf)
        if up % 2 == 0:
            assert half[fc == 0].all()                           # fc = 0: uf = (up - 1) / 2 is a half-integer
            assert ((g < 0) | (g > up - 1))[fc == 0.5].all()     # fc = +1/2: the peak sample lies in the next pixel
            assert half.all()
        else:
            assert not half[fc == 0].any() and (g[fc == 0] == (up - 1) // 2).all()
            if up > 1:
                assert half[fc != 0].all() and ((g >= 0) & (g <= up - 1)).all()      # 4.5 -> 4, -0.5 -> -0: inside the pixel
    # floor(x + 1/2) differs from rint on these inputs: the mutation has something to change
    assert (np.floor(pos + 0.5) != np.rint(pos)).any()


def test_nonfinite_group_reaches_every_kind_and_the_reference_ignores_them():
    c, rec = mc.case("nonfinite"), mc.table()["nonfinite"]
    pos = c["pos"].reshape(c["Np"], c["F"], c["npos"], 2)
    y, x = pos[..., 0], pos[..., 1]
    fin = np.isfinite(pos)
    with np.errstate(invalid="ignore"):
        for kind in (np.isnan, np.isposinf, np.isneginf, lambda v: np.abs(v) == mc.MAX_COORD, lambda v: np.abs(v) == mc.BELOW_MAX_COORD):
            one = kind(y) ^ kind(x)
            assert one.any() and (kind(y) & kind(x)).any(), kind
        assert mc.BELOW_MAX_COORD == 2.0 ** 30 - 64 and (pos == -mc.BELOW_MAX_COORD).any() and (pos == -mc.MAX_COORD).any()
    ok = mc.valid(c)
    assert ok[0].all() and ok[1].sum() == c["F"] * c["npos"] - 1 and not ok[1, 0, 1] and fin[1, 0, 1, 1]
    # just below 2^30 passes the kernel's finiteness test and is culled by every tile; at 2^30 it does not pass
    below = (np.abs(pos) == mc.BELOW_MAX_COORD).any(axis=-1) & (np.abs(pos) < mc.MAX_COORD).all(axis=-1)
    assert below.any() and ok[below].all()
    assert {k[1:3] for k in mc.survivors(c)} <= {(0, 0), (0, 1), (1, 0), (1, 1)}
    cov, win = mc.coverage(c)
    assert {p for p, _, _ in win} == {0, 1}
    # the neighbours are unchanged: the reference equals that of the two finite particles alone
    alone = mc._case("alone", "nonfinite", c["H"], c["W"], c["up"], c["sigma"], c["radius"], c["pos"][:2], c["amp"][:2])
    alone["pos"][1, 1, 0] = 500.0                                # the NaN sub-position, moved out of the field instead
    assert np.array_equal(mc.reference(alone), rec["ref"]) and rec["ref"].max() > 1


def test_lifetimes_group_reaches_every_kind():
    c = mc.case("lifetimes")
    F = c["F"]
    spans = set(zip(c["first"].tolist(), c["last"].tolist()))
    assert F == 3 and spans >= {(-2, -1), (F + 1, F + 1), (1, 1), (0, F - 1), (F - 1, F - 1)}
    ok = mc.valid(c)
    assert not ok[0].any() and not ok[1].any() and ok[3].all()
    assert [bool(ok[2, f].all()) for f in range(F)] == [False, True, False]
    assert [bool(ok[4, f].all()) for f in range(F)] == [False, False, True]
    assert not np.array_equal(mc.valid(c, "last_exclusive"), ok)


def test_far_group_reaches_the_end_of_the_field_and_both_spacings():
    far, org = mc.case("far-2^20"), mc.case("far-origin")
    assert (far["H"], far["W"]) == (2, 2 ** 20 + 70) and far["W"] <= 1 << 24
    x = far["pos"][..., 1].astype(np.float64)
    assert x[:6].min() >= far["W"] - 100 and x[:6].max() > 2 ** 20 and int(np.rint(x[:6].max())) + far["radius"] >= far["W"]
    assert x[6:].min() < 2 ** 19 < x[6:].max()
    sp = np.spacing(far["pos"][..., 1])
    assert set(sp.ravel()) == {1 / 32, 1 / 16, 1 / 8}            # below 2^19, between 2^19 and 2^20, above 2^20
    # the same scene: positions differ by the integer bases exactly, amplitudes are equal
    shift = np.where(np.arange(12)[:, None] < 6, far["reach"]["bases"][0] - org["reach"]["bases"][0],
                     far["reach"]["bases"][1] - org["reach"]["bases"][1])
    assert np.array_equal(far["pos"][..., 1].astype(np.float64), org["pos"][..., 1].astype(np.float64) + shift)
    assert np.array_equal(far["pos"][..., 0], org["pos"][..., 0]) and np.array_equal(far["amp"], org["amp"])
    rf, ro = mc.table()["far-2^20"], mc.table()["far-origin"]
    assert [(a.stop - a.start, b.start) for a, b in mc.far_regions()] == [(100, 0), (116, 120)] and mc.far_regions()[0][0].stop == far["W"]
    for a, b in mc.far_regions():
        assert rf["B"][:, :, a].max() > 1
        # the yardstick is bitwise the same at both places: nothing in the kernel's arithmetic sees the size of the coordinate
        assert np.array_equal(rf["yard"][:, :, a], ro["yard"][:, :, b])
    assert mc.c_arg("far-2^20") == mc.c_arg("far-origin")


# ---- the model ----------------------------------------------------------------------------------------------------------
def test_measured_constants_have_not_grown_past_the_written_ones():
    ce = mc.c_exp()
    worst = {c["id"]: mc.worst_exp(mc.table()[c["id"]]) for c in mc.cases()}
    top = max(worst, key=worst.get)
    print(f"c_exp = {ce:.3e} = {ce / mc.U32:.2f} roundings ({top}), written {mc.C_EXP_WRITTEN / mc.U32:.2f}")
    assert mc.U32 <= ce <= mc.C_EXP_WRITTEN
    assert ce >= 0.9 * mc.C_EXP_WRITTEN                           # and the written one is the measured one, not a loose cap
    ca = {c["id"]: mc.c_arg(c["id"]) for c in mc.cases()}
    for g in mc.groups():
        ids = [c["id"] for c in mc.cases() if c["group"] == g]
        k, e = max(ids, key=ca.get), max(ids, key=worst.get)
        print(f"{g:10s} c_arg <= {ca[k] / mc.U32:.2f} roundings ({k}); worst error / B where W <= B {worst[e] / mc.U32:.2f} roundings ({e})")
    assert mc.U32 <= max(ca.values()) <= mc.C_ARG_WRITTEN and max(ca.values()) >= 0.9 * mc.C_ARG_WRITTEN
    # the explicit FMA term: 2^-25 inv2s2 B
    c, rec = mc.case("grid-37x70-u1s0.3r0"), mc.table()["grid-37x70-u1s0.3r0"]
    m = rec["B"] > 0
    assert np.allclose(mc.fma_term(c, rec)[m] / rec["B"][m], 2.0 ** -25 / (2 * c["sigma"] ** 2), rtol=1e-12)


@pytest.mark.parametrize("cid", IDS)
def test_yardstick_is_inside_its_own_model_and_the_outer_bound(cid):
    rec = mc.table()[cid]
    assert np.isfinite(rec["ref"]).all() and np.isfinite(rec["yard"]).all()
    ok, rel = mc.outer_ok(rec["yard"], rec["ref"])
    assert ok, rel
    assert (rec["yerr"] <= mc.yard_model_of(rec, mc.c_arg(cid)) * (1 + 1e-12)).all()
    assert (rec["yard"][rec["ref"] == 0] == 0).all() and (rec["ref"][rec["B"] == 0] == 0).all()
    r = mc.ratio(rec["yard"], rec["ref"], mc.bar(cid))[0]
    assert r <= 1.0, r                                            # the kernel's bar is nowhere below the yardstick's model


@pytest.mark.parametrize("name", list(mc.MUTATIONS))
def test_every_planted_mutation_of_the_yardstick_exceeds_the_bar(name):
    what, cid = mc.MUTATIONS[name]
    c, rec = mc.case(cid), mc.table()[cid]
    bad = mc.yardstick32(c, name)
    r, err, b, i = mc.ratio(bad, rec["ref"], mc.bar(cid))
    print(f"{name} ({what}): caught by {cid}, worst error / bar {r:.3e} (error {err:.3e}, bar {b:.3e})")
    assert r > 1.0
    assert not np.array_equal(bad, rec["yard"].astype(np.float32))
