"""The readout-query variants of the last encoder layer (mode 1 of mivit_set_readout_rows) against the full
operators, through the C-ABI, on the same buffers.  The reference is always the existing full operator -- never the code
under test -- and every comparison is bitwise unless stated.

  mivit_attn_block_fwd_q1        the query side for the first 16 rows of a sequence; k and v for every row
  mivit_attn_out_bwd_rows        reads the rows r % S == 0 only, writes dctx in those rows only and zeros in the other rows of dz1
  mivit_attention_bwd_rows_lean  reads q in the rows that carry a gradient only

Shapes: both widths, bf16 and fp16; S in {2, 16, 17, 33, 64} (one tile, a full tile, a tail of one row, the benchmark's three
tiles, the largest fused sequence); B in {1, 5, 33} plus one B that makes a wave or a workgroup walk on: B = 1030 for the forward
(its grid is capped at 256 workgroups of 4 or 8 waves), B = 500 at S = 33 for the tile-walking backward kernels (516 tiles of 32
rows, a partial last tile, and a readout row at every one of the 32 positions of a tile: 33 b mod 32 = b mod 32).

Buffers a variant promises not to read hold NaN bit patterns there (all ones), outputs start as the same pattern: a row
promised unwritten must still hold it, a parameter gradient must be torch.equal to the full operator's, a live output row
bitwise equal.

Engine: mode 1 against mode 3 (mode 1 as it was before the readout query) on the rigs of tests/test_readout_rows_gpu.py -- out,
loss and the whole gradient arena bitwise equal after a workspace of 0xFF bytes; the eval-mode forward of mode 1 equals mode 0;
toggling 1 <-> 3 gives each mode's own launch sequence (told apart by the workspace bytes a mode leaves unwritten: the results
are equal by design)."""
import ctypes

import pytest
import torch

import engine_common as ec
import test_fused_blocks_gpu as fb
import test_readout_rows_gpu as rr
from test_engine_paths_gpu import Rig, _native, _same

pytestmark = pytest.mark.gpu

H = fb.H
S_LIST = (2, 16, 17, 33, 64)
SHAPES_FWD = [(B, S) for S in S_LIST for B in (1, 5, 33)] + [(1030, 33)]
SHAPES_BWD = [(B, S) for S in S_LIST for B in (1, 5, 33)] + [(500, 33)]
WD = [(w, dt) for w in (128, 64) for dt in ("bf16", "f16")]


def _raw(t):
    """the bits of a 16-bit or 32-bit tensor"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _eq(a, b):
    return a.shape == b.shape and bool(torch.equal(_raw(a), _raw(b)))


def _pattern(shape, dtype):
    """all-ones bits: a NaN in bf16, fp16 and fp32"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    _raw(t).fill_(-1)
    return t


def _untouched(t):
    return bool((_raw(t) == -1).all())


def _poison(t, rows):
    """a copy of t with the NaN pattern in `rows` (a boolean mask over the first dimension)"""
    c = t.clone()
    _raw(c)[rows] = -1
    return c


def _live(M, S):
    return (torch.arange(M, device="cuda") % S) == 0


# ---------------------------------------------------------------------------------------------------------------------
# attn_block_fwd, one query tile
# ---------------------------------------------------------------------------------------------------------------------
def _attn_fwd(entry, w, dt, c, B, S, with_qkv):
    E = fb.WIDTHS[w][0]
    t = fb.DT[dt]
    o = dict(ctx=_pattern((B, S, E), t), n=_pattern((B, S, E), t), rstd=_pattern((B, S), torch.float32),
             qkv=_pattern((B, S, 3 * E), t) if with_qkv else None)
    fb._call(entry, w, dt, *[fb._p(c[k]) for k in ("n", "gin", "bin", "Wqkv", "bqkv", "Wo", "bo", "gout", "bout")], B, S,
             fb._p(o["ctx"]), fb._p(o["n"]), fb._p(o["rstd"]), None, None, None, fb._p(o["qkv"]), fb._stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("with_qkv", [True, False], ids=["train", "lean"])
@pytest.mark.parametrize("B,S", SHAPES_FWD)
@pytest.mark.parametrize("w,dt", WD)
def test_attn_block_fwd_q1(w, dt, B, S, with_qkv):
    E = fb.WIDTHS[w][0]
    c = fb._cuda(fb.attn_fwd_inputs(B, S, w, dt, True, fb._seed("rq_fwd", w, dt, B, S)))
    full = _attn_fwd("mivit_attn_block_fwd", w, dt, c, B, S, with_qkv)
    got = _attn_fwd("mivit_attn_block_fwd_q1", w, dt, c, B, S, with_qkv)
    R0 = min(S, 16)                                  # the rows of query tile 0
    for k in ("ctx", "n", "rstd"):
        assert _eq(got[k][:, :R0], full[k][:, :R0]), f"{k}: a computed row differs from the full kernel"
    for k in ("ctx", "rstd"):
        assert _untouched(got[k][:, R0:]), f"{k}: a row behind tile 0 was written"
    if with_qkv:
        assert _eq(got["qkv"][:, :, E:], full["qkv"][:, :, E:]), "k|v differ"
        assert _eq(got["qkv"][:, :R0, :E], full["qkv"][:, :R0, :E]), "q of tile 0 differs"
        assert _untouched(got["qkv"][:, R0:, :E]), "q behind tile 0 was written"
        assert bool((_raw(got["n"][:, R0:]) == 0).all()), "n_out behind tile 0 is not zero"
    else:
        assert _untouched(got["n"][:, R0:]), "n_out behind tile 0 was written without a q|k|v store"


# ---------------------------------------------------------------------------------------------------------------------
# attn_out_bwd, readout rows
# ---------------------------------------------------------------------------------------------------------------------
def _attn_out(entry, w, dt, a, M, S=None):
    E = fb.WIDTHS[w][0]
    t = fb.DT[dt]
    dz1, dctx = _pattern((M, E), t), _pattern((M, E), t)
    arena = _pattern((E * E + 3 * E,), torch.float32)
    nb = fb._entry("mivit_attn_out_bwd_workspace_bytes", w, dt)(M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dims = (M,) if S is None else (M, S)
    fb._call(entry, w, dt, *[fb._p(a[k]) for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")], *dims, fb._p(dz1), fb._p(dctx),
             fb._p(arena[:E * E]), fb._p(arena[E * E:]), fb._p(arena[E * E + E:]), fb._p(arena[E * E + 2 * E:]), fb._p(ws), nb, fb._stream())
    torch.cuda.synchronize()
    return dz1, dctx, arena


@pytest.mark.parametrize("B,S", SHAPES_BWD)
@pytest.mark.parametrize("w,dt", WD)
def test_attn_out_bwd_rows(w, dt, B, S):
    M = B * S
    live = _live(M, S)
    a = fb._cuda(fb.attn_out_bwd_inputs(M, w, dt, fb._seed("rq_ao", w, dt, B, S)))
    a["dy"][~live] = 0                               # what the engine guarantees
    dz_f, dc_f, g_f = _attn_out("mivit_attn_out_bwd", w, dt, a, M)
    p = dict(a)
    for k in ("dy", "n1", "rstd1", "ctx"):
        p[k] = _poison(a[k], ~live)                  # rows the variant promises not to read
    dz, dc, g = _attn_out("mivit_attn_out_bwd_rows", w, dt, p, M, S)
    assert bool(torch.isfinite(g).all()) and torch.equal(g, g_f), "a parameter gradient differs from the full operator"
    assert _eq(dz[live], dz_f[live]) and _eq(dc[live], dc_f[live]), "a live row differs"
    assert _untouched(dc[~live]), "a dead row of dctx was written"
    assert bool((dz[~live] == 0).all()), "a dead row of dz1 is not zero"


# ---------------------------------------------------------------------------------------------------------------------
# attention core backward, lean
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", SHAPES_BWD)
@pytest.mark.parametrize("w,dt", WD)
def test_attention_bwd_rows_lean(w, dt, B, S):
    N = _native()
    E, _, Dh = fb.WIDTHS[w]
    t = fb.DT[dt]
    code = N.BF16 if dt == "bf16" else N.F16
    seed = fb._seed("rq_core", w, dt, B, S)
    qkv = fb.randn((B, S, 3 * E), seed, device="cuda").to(t)
    dctx = torch.zeros(B, S, E, dtype=t, device="cuda")           # the engine's layout: full rows, zero behind row 0
    dctx[:, 0] = fb.randn((B, E), seed + 1, device="cuda").to(t)
    st = fb._stream()
    ref = _pattern((B, S, 3 * E), t)
    N.check(N.lib.mivit_attention_bwd_rows(code, fb._p(qkv), fb._p(dctx), S * E, 1, B, S, H, Dh, fb._p(ref), st), "attention_bwd_rows")
    pq = qkv.clone()
    _raw(pq)[:, 1:, :E] = -1                         # q of the query rows without a gradient: they only ever multiply dS = 0
    pd = dctx.clone()
    _raw(pd)[:, 1:] = -1
    got = _pattern((B, S, 3 * E), t)
    N.check(N.lib.mivit_attention_bwd_rows_lean(code, fb._p(pq), fb._p(pd), S * E, 1, B, S, H, Dh, fb._p(got), st),
            "attention_bwd_rows_lean")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref.float()).all())
    assert _eq(got, ref), "dqkv differs from the operator that reads every q row"


# ---------------------------------------------------------------------------------------------------------------------
# engine: mode 1 (with the readout query) against mode 3 (without), eval forward, toggling
# ---------------------------------------------------------------------------------------------------------------------
class _Mode:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = _native().lib.mivit_set_readout_rows(self.value)

    def __exit__(self, *exc):
        _native().lib.mivit_set_readout_rows(self.old)


@pytest.mark.parametrize("name,B,precision", rr.PARAMS, ids=rr.IDS)
def test_mode_1_equals_mode_3(name, B, precision):
    rig = Rig(ec.CASE_BY_NAME[name], precision, B, rr._salt(name, B))
    with _Mode(3):
        old = rig.step(0xFF)
    with _Mode(1):
        new = rig.step(0xFF)
    assert bool(torch.isfinite(new.arena[~rig.pad]).all()), "mode 1 read something nobody wrote"
    assert _same(new.out, old.out) and _same(new.loss.reshape(1), old.loss.reshape(1))
    assert _same(new.arena, old.arena), "a gradient of mode 1 differs from mode 3"
    assert new.dfeat is None or _same(new.dfeat, old.dfeat)


@pytest.mark.parametrize("name,B,precision", rr.PARAMS, ids=rr.IDS)
def test_eval_forward_of_mode_1_equals_mode_0(name, B, precision):
    rig = Rig(ec.CASE_BY_NAME[name], precision, B, rr._salt(name, B))
    outs = {}
    for mode in (0, 1):
        with _Mode(mode):
            rig.ws.t.fill_(0xFF)
            rig.out.t.fill_(float("nan"))
            rig.plan.forward(rig.arena, rig.x, rig.feats, rig.B, rig.T, rig.ws.t, False, rig.out.t)
            torch.cuda.synchronize()
            outs[mode] = rig.out.t.clone()
    assert all(g.intact() for g in rig.guards)
    assert bool(torch.isfinite(outs[1]).all()) and _same(outs[0], outs[1])


@pytest.mark.parametrize("precision", ("bf16", "fp16"))
def test_toggling_1_and_3_runs_each_modes_own_launches(precision):
    """Identical arguments throughout at a graph-sized shape.  The results of modes 1 and 3 are bitwise equal by design, so the
    modes are told apart by what they leave of a workspace of 0xFF bytes: mode 3 writes the zero rows of d(ctx) and every row of the last
    layer's ctx / rstd1 / q, mode 1 does not."""
    name = "rr_w128_L2_S33"
    rig = Rig(ec.CASE_BY_NAME[name], precision, 24, rr._salt(name, 24))
    first, left = {}, {}
    for mode in (1, 3):
        with _Mode(mode):
            snaps = []
            for _ in range(3):                       # direct, captured, replayed
                snaps.append(rig.step(0xFF))
                ws = rig.ws.t.clone()
                assert mode not in left or torch.equal(ws, left[mode]), mode
                left[mode] = ws
        first[mode] = snaps[0]
        assert all(_same(s.arena, snaps[0].arena) and _same(s.out, snaps[0].out) for s in snaps[1:]), mode
    assert _same(first[1].arena, first[3].arena) and _same(first[1].out, first[3].out)
    ff = {m: int((left[m] == 0xFF).sum()) for m in left}
    assert ff[1] > ff[3] and not torch.equal(left[1], left[3]), ("the modes leave the same workspace: they cannot be told apart", ff)
    for mode in (1, 3, 1, 3):
        with _Mode(mode):
            snap = rig.step(0xFF)
        assert _same(snap.arena, first[mode].arena) and _same(snap.out, first[mode].out)
        assert torch.equal(rig.ws.t, left[mode]), f"mode {mode} ran the other mode's launches"
