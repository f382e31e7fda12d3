"""fp64 reference, fp32 yardstick, error model, restatement of the kernel's integer arithmetic, case table and planted
mutations of tests/test_movie_render.py (CPU) and tests/test_movie_render_gpu.py (csrc/movie.hip, mivit_render_movie, and its
callers helpers/generation.render_movie and simulate_movie).  numpy, and torch only to call the reference.

Reference: helpers/generation.render_movie on CPU tensors, fp64, truncation to the window included
(tests/test_movie_sim.py holds it to the naive full-grid loop; tests/test_movie_render.py does so on two table entries).

Error model, that of tests/render_common.py.  A stored pixel is v = sum_q a_q py_q[y] px_q[x] over the (particle,
sub-position) pairs q whose window holds the pixel, a profile value the mean of `up` exponentials exp(arg).  In fp32 an
exponential carries its own relative error plus the absolute error of its argument, a few roundings of |arg|, so

    E[y, x] = c_exp B + c_arg W + U,
    B = sum_q |a_q| py px,   W = the same sum with every fine sample weighted by its |arg| (rows + columns),
    U = 2^-126 (1 + A),  A = sum_q |a_q|:  below the smallest normal fp32 number an exponential, a profile or a product has an
        absolute error of at most 2^-126 each (__expf flushes; py * px may underflow where fp64 does not), times |a_q|.

c_exp and c_arg are measured on the yardstick (yardstick32: the kernel's arithmetic in numpy fp32, np.exp, unfused,
d*d - dpk*dpk as the kernel writes it, pixels accumulated in the kernel's order) against the reference:
    c_exp = the worst (|yardstick - ref| - U) / B over ALL table pixels with W <= B, never below one fp32 rounding;
    c_arg = per case, the smallest constant with |yardstick - ref| <= c_exp B + c_arg W + U on every pixel, never below
            one rounding.
Measured (asserted not to grow by tests/test_movie_render.py::test_measured_constants):
    c_exp = 17.6 roundings (1.05e-6), the worst pixel in npos-256: 512 pairs of two particles land on the same pixels, and
            the fp32 sum of n terms carries up to n - 1 roundings of B; every other group stays below 6.6 roundings;
    c_arg <= 3.9 roundings (2.3e-7), the worst case npos-256; one rounding (the floor) in chunk, cull, far, ring, ties.
The kernel gets

    bar = MARGIN (c_exp B + c_arg W) + FLOOR_ROUNDINGS 2^-24 B + U + FMA,

MARGIN = 4 (operators_common.measured_bar's margin for transcendental kernels) and FLOOR_ROUNDINGS = 4 from
render_common.  FMA: if the compiler contracts d*d - dpk*dpk into fma(d, d, -(dpk*dpk)), the square of dpk is rounded
and the square of d is not, so the two no longer cancel where d == dpk: the argument of every sample moves by at most
the rounding of dpk^2 <= 1/4, i.e. 2^-24 / 4 = 2^-26, times inv2s2.  exp' = exp, so every sample, every profile value
changes by at most that RELATIVE amount, a product of two profiles by twice it: FMA = 2^-25 inv2s2 B.  It is a term of
its own because at the peak sample |arg| = 0 and c_arg W grants nothing there.  The old bound 2e-5 * max|ref| of
tests/test_movie_sim_gpu.py stays as an outer check per case.

Two requirements of the table cannot both be met: a chunk case of 512 pairs with npos in {1, 3, 5, 7} needs 512 particles
(512 is a power of two), above the table's limit of 300.  chunk-512 therefore has 256 particles of npos = 2; the pair
count, which is what the case is about, is kept.  Likewise batch-256 fills its chunk with survivors, so no culled pair
can stand in front of them within 300 particles; every other batch case has them.
"""
import functools

import numpy as np
import torch

from render_common import FLOOR_ROUNDINGS, MARGIN, OUTER, TINY32, U32, fit_c_arg, outer_ok, ratio  # noqa: F401
from moleculardiffusion_mivit_amd.helpers import generation as gen

TH, TW = 32, 64              # csrc/movie.hip: MV_TH, MV_TW
CHUNK = 256                  # MV_CHUNK
BATCH = 64                   # MV_BATCH
MAX_COORD = 2.0 ** 30        # MV_MAX_COORD
FLT_MAX = float(np.finfo(np.float32).max)
BELOW_MAX_COORD = float(np.nextafter(np.float32(MAX_COORD), np.float32(0)))

# the measured constants as written in the docstring and in DESIGN.md 2c, rounded up in the last digit given
C_EXP_WRITTEN = 17.6 * U32
C_ARG_WRITTEN = 3.9 * U32
LIMITS = dict(Np=300, F=3)

f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _case(cid, group, H, W, up, sigma, radius, pos, amp, first=None, last=None, **reach):
    pos, amp = np.ascontiguousarray(pos, f32), np.ascontiguousarray(amp, f32)
    Np, F, npos = amp.shape
    assert pos.shape == (Np, F * npos, 2), (cid, pos.shape, amp.shape)
    sigma = float(f32(sigma))
    radius = gen.default_movie_radius(sigma, up) if radius is None else int(radius)
    if first is not None:
        first, last = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(last, np.int32)
        assert first.shape == last.shape == (Np,)
    return dict(id=cid, group=group, H=int(H), W=int(W), up=int(up), sigma=sigma, radius=radius, pos=pos, amp=amp, first=first,
                last=last, Np=Np, F=F, npos=npos, reach=reach)


def _walk(rng, start, F, npos, step=0.3):
    """[Np, F * npos, 2]: a small random walk from every start"""
    steps = step * rng.standard_normal((len(start), F * npos, 2))
    steps[:, 0] = 0
    return np.asarray(start, np.float64)[:, None, :] + np.cumsum(steps, axis=1)


def _amps(rng, Np, F, npos):
    return 100 + 10 * rng.standard_normal((Np, F, npos))


GRID_FIELDS = [(37, 70), (33, 65), (32, 64), (1, 1), (1, 200), (70, 3)]
GRID_SETTINGS = [(1, 0.3, 0), (1, 1.3, None), (2, 0.6, 4), (5, 6.5, None), (5, 1.5, 8), (4, 12.0, 16), (5, 15.0, 64), (64, 83.0, 8)]
CHUNK_CASES = [(255, 5), (256, 1), (257, 1), (512, 2), (513, 3)]          # (pairs, npos); 512: see the module docstring
BATCH_SURVIVORS = [1, 63, 64, 65, 128, 129, 256]


def _grid_cases():
    out = []
    for fi, (H, W) in enumerate(GRID_FIELDS):
        for si, (up, sigma, radius) in enumerate(GRID_SETTINGS):
            rng = np.random.default_rng(1000 + 10 * fi + si)
            start = rng.uniform([-1.5, -1.5], [H + 0.5, W + 0.5], (5, 2))
            start[0] = rng.uniform([0, 0], [H - 1, W - 1])        # one particle starts inside whatever the field and the radius
            rname = "d" if radius is None else str(radius)
            out.append(_case(f"grid-{H}x{W}-u{up}s{sigma:g}r{rname}", "grid", H, W, up, sigma, radius, _walk(rng, start, 2, 2),
                             _amps(rng, 5, 2, 2)))
    return out


def _npos_cases():
    out = []
    for npos, Np, F in ((1, 12, 2), (5, 10, 2), (7, 37, 2), (256, 2, 1)):
        rng = np.random.default_rng(2000 + npos)
        start = rng.uniform([0, 0], [36, 69], (Np, 2))
        out.append(_case(f"npos-{npos}", "npos", 37, 70, 5, 6.5, None, _walk(rng, start, F, npos), _amps(rng, Np, F, npos)))
    return out


def _chunk_cases():
    """every pair in rows 3 .. 26, columns 3 .. 55 (windows of radius 2 end at row 28, column 57), except the LAST pair, at
    (33.3, 66.4): its window (rows 31 .. 35, columns 64 .. 68) is lit by nothing else"""
    out = []
    for pairs, npos in CHUNK_CASES:
        assert pairs % npos == 0
        Np = pairs // npos
        rng = np.random.default_rng(3000 + pairs)
        pos = rng.uniform([3, 3], [26, 55], (Np, npos, 2))
        pos[-1, -1] = (33.3, 66.4)
        out.append(_case(f"chunk-{pairs}", "chunk", 37, 70, 5, 3.0, 2, pos, _amps(rng, Np, 1, npos), pairs=pairs))
    return out


def _batch_layout(n):
    """True = survivor of tile (0, 0), False = a pair that only tile (1, 1) sees, in list order"""
    if n == 256:
        return [True] * 256
    if n == 129:
        return [False, True] * 127 + [True, True]
    return [False, True] * n


def _batch_cases():
    """radius 1.  Survivors of tile (0, 0) on the lattice (1 + 2 i, 1 + 2 j), i < 15, j < 31, jittered by less than 0.3: the
    windows overlap, the centre pixel of each is its own, and none reaches row 32 or column 64.  The culled pairs sit at rows
    34 .. 35, columns 66 .. 68 and are seen by tile (1, 1) alone."""
    out = []
    lattice = np.array([(1 + 2 * i, 1 + 2 * j) for i in range(15) for j in range(31)], np.float64)
    layouts = [(f"batch-{n}", _batch_layout(n), n) for n in BATCH_SURVIVORS] + [("batch-lane255", [False] * 255 + [True], 1)]
    for k, (cid, layout, n) in enumerate(layouts):
        rng = np.random.default_rng(4000 + k)
        pos = np.zeros((len(layout), 1, 2))
        surv = np.flatnonzero(layout)
        assert len(surv) == n
        pos[surv, 0] = lattice[rng.permutation(len(lattice))[:n]] + rng.uniform(-0.3, 0.3, (n, 2))
        cull = np.flatnonzero(~np.asarray(layout))
        pos[cull, 0] = rng.uniform([33.6, 65.6], [35.4, 68.4], (len(cull), 2))
        out.append(_case(cid, "batch", 37, 70, 5, 1.5, 1, pos, _amps(rng, len(layout), 1, 1), survivors=n))
    return out


CULL_FRACTIONS = [0.3, -0.2, 0.45, -0.45]


def _cull_cases():
    """Eight particles per case, one window each, all disjoint.  `iy` / `ix` are the rounded coordinates that put one inequality
    of the cull predicate at equality or one pixel short of it; the other coordinate keeps the windows apart."""
    out = []
    for rname, radius in (("0", 0), ("3", 3), ("d", None)):
        r = gen.default_movie_radius(6.5, 5) if radius is None else radius
        assert r <= 8
        fr = np.array(CULL_FRACTIONS + CULL_FRACTIONS)
        # against the field's border: a field of exactly one tile, so that tile end and border coincide
        iy = [-r, -r - 1, 32 + r, 31 + r, 16, 5, 5, 16]
        ix = [8, 25, 42, 59, -r, -r - 1, 64 + r, 63 + r]
        pos = np.stack([np.array(iy) + fr, np.array(ix) + fr[::-1]], axis=1)[:, None, :]
        out.append(_case(f"cull-border-r{rname}", "cull", 32, 64, 5, 6.5, radius, pos, _amps(np.random.default_rng(5000 + r), 8, 1, 1),
                         at="border"))
        # against the tile seam at row 32 / column 64, in a field of 4 x 2 tiles
        iy = [32 + r, 31 + r, 32 - r, 31 - r, 6, 58, 75, 92]
        ix = [8, 25, 42, 59, 64 + r, 63 + r, 64 - r, 63 - r]
        pos = np.stack([np.array(iy) + fr, np.array(ix) + fr[::-1]], axis=1)[:, None, :]
        out.append(_case(f"cull-seam-r{rname}", "cull", 100, 81, 5, 6.5, radius, pos, _amps(np.random.default_rng(5100 + r), 8, 1, 1),
                         at="seam"))
    return out


def _ring_cases():
    pos = np.array([[[17.3, 35.8]]])
    amp = np.array([[[100.0]]])
    return [_case("ring-r3", "ring", 37, 70, 5, 6.5, 3, pos, amp), _case("ring-default", "ring", 37, 70, 5, 6.5, None, pos, amp)]


def _amps_cases():
    out = []
    walk = np.array([[0.0, 0.0], [0.4, -0.3]])
    for name, a, b in (("disjoint", (10.2, 15.3), (26.4, 50.1)), ("overlap", (15.2, 30.3), (18.4, 34.1))):
        pos = np.array([a, b])[:, None, :] + walk[None]
        amp = np.array([[[1e4, 0.9e4]], [[1e-2, 1.1e-2]]])
        out.append(_case(f"amps-{name}", "amps", 37, 70, 5, 6.5, None, pos, amp))
    rng = np.random.default_rng(6000)
    pos = _walk(rng, rng.uniform([3, 3], [33, 66], (6, 2)), 2, 2)
    amp = _amps(rng, 6, 2, 2)
    amp[0, 0, 1] = 0.0
    amp[1] = 0.0                                 # a whole particle of exact zeros
    amp[2, 1, 0] = -0.0
    amp[3, 0, 0] = -80.0                         # a negative value among positive ones
    out.append(_case("amps-signs", "amps", 37, 70, 5, 6.5, None, pos, amp))
    pos = _walk(rng, rng.uniform([3, 3], [33, 66], (5, 2)), 2, 2)
    amp = _amps(rng, 5, 2, 2)
    amp[0, 0, 1] = np.inf
    amp[1, 1, 0] = np.nan
    amp[2, 0, 0] = -np.inf
    amp[3, :, :] = np.nan
    out.append(_case("amps-nonfinite", "amps", 37, 70, 5, 6.5, None, pos, amp))
    return out


TIE_POSITIONS = [(5.0, 5.0), (5.5, 14.5), (6.5, 24.5), (14.0, 33.5), (14.5, 43.0), (15.5, 52.5), (23.0, 7.0), (23.5, 17.5),
                 (31.5, 63.5), (22.5, 28.5), (4.5, 62.5), (32.5, 44.5)]


def _ties_cases():
    """radius 3, so that the window rint chooses is visible at its edge.  (31.5, 63.5) rounds to (32, 64): the tie decides the
    tile.  Every coordinate is k or k + 1/2, exact in fp32."""
    out = []
    pos = np.array(TIE_POSITIONS)[:, None, :]
    for up, sigma in ((1, 0.8), (2, 1.2), (4, 3.0), (5, 4.0)):
        out.append(_case(f"ties-u{up}", "ties", 37, 70, up, sigma, 3, pos, _amps(np.random.default_rng(7000 + up), len(pos), 1, 1)))
    return out


def _nonfinite_case():
    rng = np.random.default_rng(8000)
    n, i, b, m = np.nan, np.inf, BELOW_MAX_COORD, MAX_COORD
    special = [(n, 20.0), (20.0, i), (-i, -i), (b, 30.0), (m, 30.0), (-m, -m), (12.0, -b), (b, b), (n, n), (15.0, -i), (-b, 40.0), (i, i)]
    Np = 2 + len(special)
    pos = _walk(rng, rng.uniform([3, 3], [33, 66], (Np, 2)), 2, 2)
    for k, v in enumerate(special):
        pos[2 + k] = v
    pos[1, 1, 0] = n                             # one NaN sub-position (frame 0, s = 1, y only) inside a visible particle
    return _case("nonfinite", "nonfinite", 37, 70, 5, 6.5, None, pos, _amps(rng, Np, 2, 2))


def _lifetimes_case():
    rng = np.random.default_rng(9000)
    F = 3
    first = [-2, F + 1, 1, 0, F - 1, 0, 0]
    last = [-1, F + 1, 1, F - 1, F - 1, 0, 1]
    Np = len(first)
    pos = _walk(rng, rng.uniform([3, 3], [33, 66], (Np, 2)), F, 2)
    return _case("lifetimes", "lifetimes", 37, 70, 5, 6.5, None, pos, _amps(rng, Np, F, 2), first, last)


FAR_W = 2 ** 20 + 70
FAR_BASES = (2 ** 20 - 30, 2 ** 19 - 50)         # the last 100 columns of the field; around column 2^19
FAR_ORIGIN_BASES = (0, 128)
FAR_SPAN = 100


def _far_cases():
    """Offsets rounded to 1/8, so that base + offset is exact in fp32 up to 2^21 (spacing 1/8 above 2^20, 1/16 and 1/32 on
    the two sides of 2^19): the far scene and the origin scene are the same scene."""
    rng = np.random.default_rng(10000)
    off = np.round(_walk(rng, rng.uniform([-1.0, 0.0], [2.0, FAR_SPAN - 0.5], (12, 2)), 1, 2) * 8) / 8
    off[..., 1] = np.clip(off[..., 1], 0.0, FAR_SPAN - 0.125)
    off[0, :, 1] = (97.25, FAR_SPAN - 0.125)     # one particle's window passes the last column of the field
    amp = _amps(rng, 12, 1, 2)
    out = []
    for cid, W, bases in (("far-2^20", FAR_W, FAR_BASES), ("far-origin", 256, FAR_ORIGIN_BASES)):
        pos = off.copy()
        pos[:6, :, 1] += bases[0]
        pos[6:, :, 1] += bases[1]
        assert (pos.astype(f32).astype(np.float64) == pos).all()
        out.append(_case(cid, "far", 2, W, 5, 6.5, None, pos, amp, bases=bases))
    return out


def far_regions():
    """[(columns of far-2^20, the same columns of far-origin)] per cluster: the windows of a cluster, cut where either field ends"""
    out = []
    for bf, bo in zip(FAR_BASES, FAR_ORIGIN_BASES):
        lo, hi = -min(8, bo), min(FAR_SPAN + 8, FAR_W - bf)
        out.append((slice(bf + lo, bf + hi), slice(bo + lo, bo + hi)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = (_grid_cases() + _npos_cases() + _chunk_cases() + _batch_cases() + _cull_cases() + _ring_cases() + _amps_cases()
           + _ties_cases() + [_nonfinite_case(), _lifetimes_case()] + _far_cases())
    assert len({c["id"] for c in out}) == len(out)
    assert all(c["Np"] <= LIMITS["Np"] and c["F"] <= LIMITS["F"] for c in out)
    return tuple(out)


def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def groups():
    return sorted({c["group"] for c in cases()})


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's integer arithmetic, restated (csrc/movie.hip:67-93)
# ---------------------------------------------------------------------------------------------------------------------
def valid(c, mut=None):
    """[Np, F, npos] bool: visible in the frame, position and amplitude finite, |coordinate| < 2^30 (movie.hip:74-77)"""
    Np, F, npos = c["amp"].shape
    pos = c["pos"].reshape(Np, F, npos, 2)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(pos) < MAX_COORD).all(axis=-1) & (np.abs(c["amp"]) <= FLT_MAX)
    if c["first"] is not None:
        fr = np.arange(F)[None, :, None]
        la = c["last"][:, None, None]
        ok &= (c["first"][:, None, None] <= fr) & ((fr < la) if mut == "last_exclusive" else (fr <= la))
    return ok


def centres(c):
    """[Np, F, npos, 2] int64: (iy, ix) = rint of the fp32 position, 0 where it is not finite"""
    Np, F, npos = c["amp"].shape
    pos = c["pos"].reshape(Np, F, npos, 2)
    with np.errstate(invalid="ignore"):
        fin = np.abs(pos) < MAX_COORD
    return np.rint(np.where(fin, pos, 0)).astype(np.int64)


def margins(iy, ix, r, y0, x0):
    """lhs - rhs of the four inequalities of movie.hip:79, and whether each holds"""
    d = (iy + r - y0, iy - r - (y0 + TH), ix + r - x0, ix - r - (x0 + TW))
    return d, (d[0] >= 0, d[1] < 0, d[2] >= 0, d[3] < 0)


def tiles(c):
    return (c["H"] + TH - 1) // TH, (c["W"] + TW - 1) // TW


def survivors(c):
    """{(f, tileY, tileX, chunk): [index within the chunk (= thread) of every surviving pair, ascending]}"""
    ok, cen, r = valid(c), centres(c), c["radius"]
    tilesY, tilesX = tiles(c)
    out = {}
    Np, F, npos = c["amp"].shape
    for f in range(F):
        for p in range(Np):
            for s in range(npos):
                if not ok[p, f, s]:
                    continue
                q = p * npos + s
                iy, ix = int(cen[p, f, s, 0]), int(cen[p, f, s, 1])
                for tY in range(max(0, (iy - r) // TH - 1), min(tilesY - 1, (iy + r) // TH + 1) + 1):
                    for tX in range(max(0, (ix - r) // TW - 1), min(tilesX - 1, (ix + r) // TW + 1) + 1):
                        if all(margins(iy, ix, r, tY * TH, tX * TW)[1]):
                            out.setdefault((f, tY, tX, q // CHUNK), []).append(q % CHUNK)
    return out


def window(ic, r, n):
    """the pixels lo .. hi - 1 of a window of radius r about ic inside a field side of n"""
    return max(ic - r, 0), min(ic + r, n - 1) + 1


def coverage(c):
    """[F, H, W] int: how many valid pairs' windows hold the pixel; and {(p, f, s): (ylo, yhi, xlo, xhi)}"""
    ok, cen, r = valid(c), centres(c), c["radius"]
    cov = np.zeros((c["F"], c["H"], c["W"]), np.int32)
    win = {}
    for p, f, s in zip(*np.nonzero(ok)):
        ylo, yhi = window(int(cen[p, f, s, 0]), r, c["H"])
        xlo, xhi = window(int(cen[p, f, s, 1]), r, c["W"])
        if ylo < yhi and xlo < xhi:
            cov[f, ylo:yhi, xlo:xhi] += 1
            win[(int(p), int(f), int(s))] = (ylo, yhi, xlo, xhi)
    return cov, win


# ---------------------------------------------------------------------------------------------------------------------
# fp64: reference and magnitudes
# ---------------------------------------------------------------------------------------------------------------------
def reference(c):
    t = lambda a: None if a is None else torch.from_numpy(a)      # noqa: E731
    out = gen.render_movie(torch.from_numpy(c["pos"]), torch.from_numpy(c["amp"]), c["sigma"], c["H"], c["W"], c["up"], c["radius"],
                           t(c["first"]), t(c["last"]))
    assert out.dtype == torch.float64
    return out.numpy()


def prof64(cc, idx, up, sigma):
    """prof(i; c) of the definition for the pixels idx, and the same mean with every sample weighted by its |arg|"""
    u = cc * up + (up - 1) / 2.0
    dpk = np.rint(u) - u
    d = (idx[:, None] * up + np.arange(up)) - u
    arg = -(d * d - dpk * dpk) / (2.0 * sigma * sigma)
    e = np.exp(arg)
    return e.mean(axis=1), (e * np.abs(arg)).mean(axis=1)


def magnitudes(c):
    """-> B, W, A [F, H, W] fp64, see the module docstring"""
    ok, cen, r = valid(c), centres(c), c["radius"]
    Np, F, npos = c["amp"].shape
    pos = c["pos"].reshape(Np, F, npos, 2).astype(np.float64)
    B = np.zeros((F, c["H"], c["W"]))
    Wt, A = np.zeros_like(B), np.zeros_like(B)
    with np.errstate(under="ignore"):
        for p, f, s in zip(*np.nonzero(ok)):
            ylo, yhi = window(int(cen[p, f, s, 0]), r, c["H"])
            xlo, xhi = window(int(cen[p, f, s, 1]), r, c["W"])
            if ylo >= yhi or xlo >= xhi:
                continue
            py, pyA = prof64(pos[p, f, s, 0], np.arange(ylo, yhi, dtype=np.float64), c["up"], c["sigma"])
            px, pxA = prof64(pos[p, f, s, 1], np.arange(xlo, xhi, dtype=np.float64), c["up"], c["sigma"])
            a = abs(float(c["amp"][p, f, s]))
            B[f, ylo:yhi, xlo:xhi] += a * py[:, None] * px[None, :]
            Wt[f, ylo:yhi, xlo:xhi] += a * (pyA[:, None] * px[None, :] + py[:, None] * pxA[None, :])
            A[f, ylo:yhi, xlo:xhi] += a
    return B, Wt, A


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick: the kernel's arithmetic in numpy fp32, and planted defects of it
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # name: (the planted defect, the table case that must catch it)
    "window_short": ("the window one ring short", "ring-default"),
    "window_wide": ("the window one ring wide", "ring-r3"),
    "tail_chunk": ("the pairs of the last, partial chunk dropped", "chunk-257"),
    "survivor_65": ("the 65th survivor of a (tile, chunk) dropped", "batch-65"),
    "floor_half": ("rint replaced by floor(x + 0.5)", "ties-u5"),
    "no_dpk": ("dpk dropped from the argument", "grid-37x70-u2s0.6r4"),
    "amp_shift": ("the amplitude of sub-position s taken from s - 1", "npos-5"),
    "last_exclusive": ("first <= f < last", "lifetimes"),
    "swap_yx": ("(y, x) swapped", "npos-1"),
}


def _prof32(cc, r, n, up, inv2s2, mut):
    """-> lo, hi, fp32 profile of the pixels lo .. hi - 1 (movie.hip:105-118)"""
    rnd = (lambda v: np.floor(v + f32(0.5))) if mut == "floor_half" else np.rint
    ic = rnd(cc)
    lo, hi = window(int(ic), r, n)
    if lo >= hi:
        return lo, hi, None
    di = np.arange(lo, hi) - int(ic)
    uf = (cc - ic) * f32(up) + f32(0.5) * f32(up - 1)
    dpk = f32(0) if mut == "no_dpk" else rnd(uf) - uf
    base = (di * up).astype(f32) - uf
    acc = np.zeros(len(di), f32)
    for k in range(up):
        d = base + f32(k)
        acc += np.exp(-(d * d - dpk * dpk) * inv2s2)
    assert acc.dtype == f32 and uf.dtype == f32
    return lo, hi, acc * (f32(1) / f32(up))


def yardstick32(c, mut=None):
    assert mut is None or mut in MUTATIONS
    Np, F, npos = c["amp"].shape
    pos = c["pos"].reshape(Np, F, npos, 2)
    ok = valid(c, mut)
    r = c["radius"] + {"window_short": -1, "window_wide": 1}.get(mut, 0)
    inv2s2 = f32(1) / (f32(2) * f32(c["sigma"]) * f32(c["sigma"]))
    pairs = Np * npos
    dropped = {}
    if mut == "survivor_65":
        for (f, tY, tX, ch), tids in survivors(c).items():
            if len(tids) > BATCH:
                dropped.setdefault((f, ch * CHUNK + tids[BATCH]), []).append((tY, tX))
    out = np.zeros((F, c["H"], c["W"]), f32)
    with np.errstate(under="ignore"):
        for f in range(F):
            for q in range(pairs):                                   # particles ascending, sub-positions ascending
                p, s = divmod(q, npos)
                if not ok[p, f, s] or r < 0:
                    continue
                if mut == "tail_chunk" and pairs > CHUNK and q >= (pairs - 1) // CHUNK * CHUNK:
                    continue
                cy, cx = pos[p, f, s, ::-1] if mut == "swap_yx" else pos[p, f, s]
                a = c["amp"][p, f, max(s - 1, 0)] if mut == "amp_shift" else c["amp"][p, f, s]
                ylo, yhi, py = _prof32(cy, r, c["H"], c["up"], inv2s2, mut)
                xlo, xhi, px = _prof32(cx, r, c["W"], c["up"], inv2s2, mut)
                if py is None or px is None:
                    continue
                blk = (a * py)[:, None] * px[None, :]                # the amplitude folded into the row profile
                for tY, tX in dropped.get((f, q), ()):
                    ys = slice(max(tY * TH, ylo) - ylo, max(min(tY * TH + TH, yhi) - ylo, 0))
                    xs = slice(max(tX * TW, xlo) - xlo, max(min(tX * TW + TW, xhi) - xlo, 0))
                    blk[ys, xs] = 0
                assert blk.dtype == f32
                out[f, ylo:yhi, xlo:xhi] += blk
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the measured model
# ---------------------------------------------------------------------------------------------------------------------
def record(c):
    """dict(ref, B, W, A, U, yard, yerr) of any case, in the table or not; read-only arrays"""
    ref = reference(c)
    B, Wt, A = magnitudes(c)
    yard = yardstick32(c).astype(np.float64)
    rec = dict(ref=ref, B=B, W=Wt, A=A, U=TINY32 * (1 + A), yard=yard, yerr=np.abs(yard - ref))
    for v in rec.values():
        v.setflags(write=False)
    rec["id"] = c["id"]
    return rec


@functools.lru_cache(maxsize=None)
def table():
    """id -> record; computed once and never changed"""
    return {c["id"]: record(c) for c in cases()}


def worst_exp(rec):
    """-> (the worst (yerr - U) / B over the record's pixels with 0 < B, W <= B; 0 without any)"""
    m = (rec["B"] > 0) & (rec["W"] <= rec["B"])
    return float(((rec["yerr"][m] - rec["U"][m]) / rec["B"][m]).max()) if m.any() else 0.0


@functools.lru_cache(maxsize=None)
def c_exp():
    return max(U32, max(worst_exp(rec) for rec in table().values()))


def c_arg_of(rec):
    return fit_c_arg(rec["yerr"], rec["B"], rec["W"], rec["U"], c_exp())


@functools.lru_cache(maxsize=None)
def c_arg(cid):
    return c_arg_of(table()[cid])


def fma_term(c, rec):
    """2^-25 inv2s2 B: see the module docstring"""
    return 2.0 ** -25 / (2.0 * c["sigma"] * c["sigma"]) * rec["B"]


def yard_model_of(rec, ca):
    return c_exp() * rec["B"] + ca * rec["W"] + rec["U"]


def bar_of(c, rec, ca):
    return MARGIN * (c_exp() * rec["B"] + ca * rec["W"]) + FLOOR_ROUNDINGS * U32 * rec["B"] + rec["U"] + fma_term(c, rec)


def bar(cid):
    """per pixel: what the code under test may be off by"""
    return bar_of(case(cid), table()[cid], c_arg(cid))


def bar_for(c):
    """-> ref, bar of a case outside the table: the table's c_exp, c_arg fitted on this case's own yardstick"""
    rec = record(c)
    return rec["ref"], bar_of(c, rec, c_arg_of(rec))
