"""The operator level of the C-ABI -- mivit_linear_fwd / _dgrad / _wgrad (csrc/gemm.hip) and mivit_layernorm_fwd / _bwd
(csrc/norm.hip) -- called directly with the arguments `ops.py` never sets: strides, misaligned pointers, fp32 rows in the 16-bit
modes, the residual / y_preact / act'(saved) / dres epilogues, accumulate, NULL outputs, the LayerNorm row map and `pos`.

Rounding model (fp64 references in tests/operators_common.py, `rnd` = rounding to the element type T, nothing in fp32 mode):
  * linear_fwd.  Operands enter LDS as T: an fp32 x and the fp32 W are rounded while staged (gemm.hip:84-99 `pack2` /
    `store_lds`, :125-133).  Products accumulate in fp32 (MFMA, :233); the bias is added in fp32 (:261, :301); y_preact =
    rnd(acc + bias) (:264, :315, :336); y = rnd(act(acc + bias) + resid) with act on the unrounded fp32 value (:265-269,
    :317-330, :337-340).
  * linear_dgrad.  dx = rnd((dy @ rnd(W)) * act'(saved) + dres) (:266-267, :318-329); act' from common.h:80-90: relu and
    leaky (slope 0.01) test `saved > 0` strictly on the post-activation, gelu takes the pre-activation.
  * linear_wgrad.  dW (+)= dy^T @ rnd(x), db (+)= column sums of dy, fp32 (gemm.hip:483-534, misc.hip:100-156).
  * layernorm_fwd.  mean, biased variance (two passes), rstd = rsqrt(var + 1e-5) in fp32; y[map(r)] = rnd((z - mu) * rstd *
    gamma + beta + pos[map(r) % out_seq_stride]) (norm.hip:39-56, :172-193); mean[r] / rstd[r] unmapped.
  * layernorm_bwd.  xh = (z - mean) * rstd, g = dy * gamma, dz = rnd(rstd * (g - mean(g) - xh * mean(g xh))), dgamma (+)= sum
    dy xh, dbeta (+)= sum dy (:96-117, :229-266); dy is read at map(r), z / dz at r.  The kernel is given the mean / rstd of
    the reference, so the two directions are tested independently.

Two kinds of assertion.  EXACT: small-integer operands ((i*7 + j*3 + ...) % 5 - 2 and the like) whose every result is an
integer of the element type -- torch.equal against the integer reference for every placement property.  For LayerNorm the
exact part is placement: mapped / strided output rows bitwise equal to the contiguous run of the same kernel, `pos` against
the run without it (fp32: fl(y + pos) bitwise; 16-bit: gamma = 0, integer beta, power-of-two pos).  ACCURACY: random operands,
|got - ref| against a bar, element by element (sharper than a row's largest error against the row's largest bar: a small
element may not be off by half an ulp of a large one); ref = the UNROUNDED fp64 value, the bar of an element:
  1. final rounding: half an ulp of T at the element, 2^(floor(log2 |x|) - p), p = 8 (bf16) / 11 (fp16) -- between 2^-9 and
     2^-8 of |x| in bf16, 2^-12 .. 2^-11 in fp16; 0 for fp32 outputs;
  2. fp32 arithmetic: GEMMs K_red * 2^-24 * (|A| @ |B|) on the staged values, K_red = reduction length + slab count, x 2
     where bias / activation / residual follow (an accumulate adds |prefill| inside the bracket); gelu and LayerNorm:
     4 x the worst per-row error of the fp32 restatement of the same formulas (the reference functions run in torch fp32 on
     the CPU) relative to the row's largest magnitude, measured on the test's own inputs and never taken below one fp32
     rounding, 2^-24.
     One deviation, for LayerNorm's y on rows of variance below 1/64 (rstd > 8) only: there the yardstick term is never
     below one fp32 rounding of the row's mean carried into y, 2^-24 * (max|y| + rstd * max|gamma| * max|z|).  y inherits the
     mean's error times rstd * gamma, and a mean good to one rounding is the most an fp32 summation promises (at E = 8 and
     variance 1e-3 the CPU restatement happens to be four times better than that, the kernel is not).  On every other row
     the bar is the 4 x yardstick alone; a CPU test asserts that the floor governs low-variance rows only.
Yardsticks measured on the CPU, worst over the cases, bf16 / fp16 / fp32 mode (`pytest -m "not gpu" -s` prints them; each test
uses the one of its own inputs): gelu forward 2.4e-7 / 5.5e-7 / 6.5e-7, gelu dgrad 2.4e-7 / 6.4e-7 / 4.1e-7, LayerNorm y
9.9e-7 / 9.9e-7 / 2.8e-6 (3.6e-5 with the 1000 +- 1 row), mean 8.0e-8 / 7.7e-8 / 1.4e-7, rstd 1.6e-7 / 1.9e-7 / 1.9e-7, dz
5.7e-7 / 6.5e-7 / 3.3e-7, dgamma 1.4e-7 / 1.8e-7 / 1.7e-7, dbeta 6.0e-8 / 6.0e-8 / 1.9e-7 of the row's scale.
Worst error / bar seen on the MI355X (the `_report_worst` fixture prints them), bf16 / fp16 / fp32 mode: linear_fwd 1.000 /
0.994 / 0.317, linear_dgrad 0.999 / 0.994 / 0.250, linear_wgrad 0.005 / 0.005 / 0.015, layernorm_fwd 1.000 / 0.998 / 0.606,
layernorm_bwd 1.000 / 0.999 / 0.446.  In the 16-bit modes the bar is almost all final rounding (7.812e-3 against 7.815e-3 for a
bf16 value in [1, 2)): a ratio of 1.000 says the worst element sat next to a rounding boundary, the fp32 column says how much
of the arithmetic term is used.  The weight gradient's bound grows with the reduction length and is far from attained.  All 571
GPU cases take 5 s, the slowest (the 64x128 tile at 24 449 rows) 0.4 s.
Memory: every strided or mapped input carries NaN in its padding columns and unmapped rows; every output carries a sentinel bit
pattern in padding columns, unmapped rows and one guard row before and after, checked bitwise after every call (`Out.read`).
Workspaces are exactly the size the query returns.

Branch coverage is asserted on the CPU by restatements of launch_gemm_t, wgrad_splits, colsum_chunks, vec_plan, ln_blocks and
the EPL / NV selection (test_*_cases_cover_every_branch).  Not reachable through the C-ABI: the `map_rows` row map of the GEMM
epilogue (engine only -- there `orow == row`), `w_is_bf16`, `y_is_f32` / `dx_is_f32`, and a single-split weight gradient with
several column-sum chunks (needs ceil(N/128) * ceil(K/128) >= 384).  No exemption is taken: the 64x128 tile runs at its
smallest shape, (24449, 128, 1024).
"""
import ctypes

import pytest
import torch

import operators_common as oc
from gpu_buffers import ITYPE, SENT, Out, inp
from operators_common import ALL, CODE, DT, ESIZE

gpu = pytest.mark.gpu
_WORST = {}     # (entry point, dtype) -> (ratio, error, bar, what)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (ep, dt), (ratio, e, b, what) in sorted(_WORST.items()):
        print(f"[operators] {ep:14s} {dt:4s} worst {e:.3e} = {ratio:.3f} of its bar {b:.3e}  ({what})")


def _note(ep, dt, what, got, ref, bar):
    ratio, e, b, row = oc.row_ratio(got, ref, bar)
    print(f"[operators] {ep} {dt} {what}: row {row} error {e:.3e} bar {b:.3e} ratio {ratio:.3f}")
    if ratio >= _WORST.get((ep, dt), (-1,))[0]:
        _WORST[(ep, dt)] = (ratio, e, b, what)
    return ratio


def _check(ep, dt, what, got, ref, bar):
    assert bool(torch.isfinite(got.double()).all()), f"{ep} {dt} {what}: non-finite output"
    ratio = _note(ep, dt, what, got, ref, bar)
    assert ratio <= 1.0, f"{ep} {dt} {what}: error is {ratio:.3f} of its bar"


def _params(cases):
    return [pytest.param(dt, c, id=f"{dt}-{c['id']}") for c in cases for dt in oc.case_dts(c)]


# ---------------------------------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------------------------------
def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _lib():
    from moleculardiffusion_mivit_amd import _native as N
    return N


# ---------------------------------------------------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------------------------------------------------
def run_fwd(dt, c, x, W, bias, resid):
    N_ = _lib()
    M, N, K = c["M"], c["N"], c["K"]
    xf32 = bool(c.get("xf32"))
    ldx, ldy = c.get("ldx", K), c.get("ldy", N)
    xb, xp = inp(x, "f32" if xf32 else dt, ldx, c.get("xo", 0))
    Wg, bg = W.cuda(), bias.cuda()
    y = Out(dt, M, N, ldy, c.get("yo", 0))
    pre = Out(dt, M, N, ldy, c.get("po", 0)) if c.get("pre") else None
    rb, rp = inp(resid, dt, c["ldr"], c.get("ro", 0)) if c.get("ldr") else (None, None)
    N_.check(N_.lib.mivit_linear_fwd(CODE[dt], xp, int(xf32), ldx, _p(Wg), _p(bg), M, N, K, c.get("act", 0), rp,
                                     c.get("ldr") or 0, y.ptr, ldy, pre.ptr if pre else None, _st()), "linear_fwd")
    torch.cuda.synchronize()
    return y.read(), pre.read() if pre else None


def run_dgrad(dt, c, dy, W, saved, dres):
    N_ = _lib()
    M, N, K = c["M"], c["N"], c["K"]
    lddy, lddx = c.get("lddy", N), c.get("lddx", K)
    act = c.get("act", 0)
    dyb, dyp = inp(dy, dt, lddy, c.get("dyo", 0))
    Wg = W.cuda()
    sb, sp = inp(saved, dt, c["lds"], c.get("so", 0)) if act else (None, None)
    rb, rp = inp(dres, dt, c["lddr"], c.get("ro", 0)) if c.get("lddr") else (None, None)
    dx = Out(dt, M, K, lddx, c.get("dxo", 0))
    N_.check(N_.lib.mivit_linear_dgrad(CODE[dt], dyp, lddy, _p(Wg), M, N, K, act, sp, c.get("lds") or 0, rp,
                                       c.get("lddr") or 0, dx.ptr, lddx, _st()), "linear_dgrad")
    torch.cuda.synchronize()
    return dx.read()


def run_wgrad(dt, c, dy, x, dW0, db0):
    """-> (dW, db) of two calls each, asserted bitwise equal (the header promises determinism)"""
    N_ = _lib()
    M, N, K = c["M"], c["N"], c["K"]
    xf32 = bool(c.get("xf32"))
    lddy, ldx = c.get("lddy", N), c.get("ldx", K)
    dyb, dyp = inp(dy, dt, lddy, c.get("dyo", 0))
    xb, xp = inp(x, "f32" if xf32 else dt, ldx, c.get("xo", 0))
    nbytes = N_.lib.mivit_linear_wgrad_workspace_bytes(M, N, K)
    assert nbytes == oc.wgrad_ws_bytes(M, N, K)
    res = []
    for _ in range(2):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN bit patterns: nothing is assumed zero
        dW = Out("f32", N, K, K, init=dW0) if c.get("dW", True) else None
        db = Out("f32", 1, N, N, init=db0[None] if db0 is not None else None) if c.get("db", True) else None
        N_.check(N_.lib.mivit_linear_wgrad(CODE[dt], dyp, lddy, xp, int(xf32), ldx, M, N, K, dW.ptr if dW else None,
                                           db.ptr if db else None, c.get("acc", 0), _p(ws), nbytes, _st()), "linear_wgrad")
        torch.cuda.synchronize()
        res.append((dW.read() if dW else None, db.read()[0] if db else None))
    for a, b in zip(*res):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32)), "wgrad is not repeatable"
    return res[0]


def _ln_geometry(c):
    M, mp = c["M"], c.get("mp")
    rows = oc.map_rows(M, mp)
    total = M if mp is None else mp[0] * (mp[1] + mp[2])
    args = (0, 0, 0) if mp is None else (mp[1], mp[1] + mp[2], mp[2])
    return rows, total, args


def run_ln_fwd(dt, c, z, gamma, beta, pos=None):
    N_ = _lib()
    M, E = c["M"], c["E"]
    rows, total, (rps, stride, off) = _ln_geometry(c)
    zb, zp = inp(z, dt, c["ldz"], c.get("zo", 0))
    y = Out(dt, total, E, c["ldy"], c.get("yo", 0), rows=rows)
    mean, rstd = Out("f32", 1, M, M), Out("f32", 1, M, M)
    gg, bg = gamma.cuda(), beta.cuda()
    pg = pos.cuda() if pos is not None else None
    N_.check(N_.lib.mivit_layernorm_fwd(CODE[dt], zp, c["ldz"], _p(gg), _p(bg), M, E, y.ptr, c["ldy"], rps, stride, off,
                                        _p(pg), mean.ptr, rstd.ptr, _st()), "layernorm_fwd")
    torch.cuda.synchronize()
    return y.read(), mean.read()[0], rstd.read()[0]


def run_ln_bwd(dt, c, dy, z, gamma, mean, rstd, dg0=None, db0=None):
    N_ = _lib()
    M, E = c["M"], c["E"]
    rows, total, (rps, stride, off) = _ln_geometry(c)
    dyb, dyp = inp(dy, dt, c["ldy"], c.get("yo", 0), rows=rows, total=total)
    zb, zp = inp(z, dt, c["ldz"], c.get("zo", 0))
    dz = Out(dt, M, E, c["lddz"], c.get("dzo", 0))
    dg = Out("f32", 1, E, E, init=dg0[None] if dg0 is not None else None) if c.get("dgamma", True) else None
    db = Out("f32", 1, E, E, init=db0[None] if db0 is not None else None) if c.get("dbeta", True) else None
    gg, mg, rg = gamma.cuda(), mean.cuda(), rstd.cuda()
    nbytes = N_.lib.mivit_layernorm_bwd_workspace_bytes(M, E)
    assert nbytes == oc.ln_bwd_ws_bytes(M, E)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    N_.check(N_.lib.mivit_layernorm_bwd(CODE[dt], dyp, c["ldy"], zp, c["ldz"], _p(gg), _p(mg), _p(rg), M, E, rps, stride, off,
                                        dz.ptr, c["lddz"], dg.ptr if dg else None, db.ptr if db else None, c.get("acc", 0),
                                        _p(ws), nbytes, _st()), "layernorm_bwd")
    torch.cuda.synchronize()
    return dz.read(), dg.read()[0] if dg else None, db.read()[0] if db else None


# ---------------------------------------------------------------------------------------------------------------------
# operands and expectations (CPU)
# ---------------------------------------------------------------------------------------------------------------------
INT_LIMIT = {"f32": 2.0 ** 24, "bf16": 256.0, "f16": 2048.0}


def fwd_int_operands(c):
    M, N, K = c["M"], c["N"], c["K"]
    x = oc.ints((M, K), 7, 3, c.get("mod", 5), c.get("lo", -2), mix=1)
    W = oc.ints((N, K), 5, 11, 3, -1, mix=1)
    return x, W, oc.ints((N,), 3, 0, 7, -3), oc.ints((M, N), 11, 5, 9, -4)


def dgrad_int_operands(c):
    M, N, K = c["M"], c["N"], c["K"]
    dy = oc.ints((M, N), 7, 3, 5, -2, mix=1)
    W = oc.ints((N, K), 5, 11, 3, -1, mix=1)
    saved = oc.ints((M, K), 3, 7, 4, -1)                 # -1, 0, 1, 2 ...
    saved[(torch.arange(M)[:, None] + torch.arange(K)[None, :]) % 5 == 0] = -0.0      # ... and -0.0
    return dy, W, saved, oc.ints((M, K), 11, 5, 9, -4)


def wgrad_int_operands(c):
    M, N, K = c["M"], c["N"], c["K"]
    return (oc.ints((M, N), 7, 3, 5, -2, mix=1), oc.ints((M, K), 5, 11, 4, -1, mix=1), oc.ints((N, K), 13, 7, 201, -100),
            oc.ints((N,), 17, 0, 201, -100))


def fwd_random_operands(dt, c):
    M, N, K = c["M"], c["N"], c["K"]
    x = oc.randn((M, K), 1, dt=None if c.get("xf32") else dt)
    return x, oc.randn((N, K), 2, K ** -0.5), oc.randn((N,), 3, 0.1), oc.randn((M, N), 4, dt=dt)


def dgrad_random_operands(dt, c):
    M, N, K = c["M"], c["N"], c["K"]
    saved = oc.randn((M, K), 7, dt=dt)
    saved[0, 0], saved[-1, -1] = 0.0, -0.0
    return oc.randn((M, N), 5, dt=dt), oc.randn((N, K), 6, N ** -0.5), saved, oc.randn((M, K), 8, dt=dt)


def wgrad_random_operands(dt, c):
    M, N, K = c["M"], c["N"], c["K"]
    return (oc.randn((M, N), 9, dt=dt), oc.randn((M, K), 10, dt=None if c.get("xf32") else dt), oc.randn((N, K), 11),
            oc.randn((N,), 12))


def fwd_bars(dt, c, x, W, bias, resid):
    """-> (y64, u64, bar_y, bar_u, yardstick or None)"""
    act = c.get("act", 0)
    r = resid if c.get("ldr") else None
    y64, u64 = oc.ref_linear_fwd(dt, x, W, bias, act, r)
    term = oc.gemm_fp32_term(oc.rnd(x, dt), oc.rnd(W, dt).t(), c["K"] + 1, 2.0)
    bar_u = oc.half_ulp(u64, dt) + term
    if act != 3:
        return y64, u64, oc.half_ulp(y64, dt) + term, bar_u, None
    y32, _ = oc.ref_linear_fwd(dt, x, W, bias, act, r, cdt=torch.float32)
    yard = oc.yardstick(y32, y64)
    return y64, u64, oc.measured_bar(y64, yard, dt), bar_u, yard


def dgrad_bars(dt, c, dy, W, saved, dres):
    act = c.get("act", 0)
    d = dres if c.get("lddr") else None
    r64 = oc.ref_linear_dgrad(dt, dy, W, act, saved, d)
    if act != 3:
        return r64, oc.half_ulp(r64, dt) + oc.gemm_fp32_term(dy, oc.rnd(W, dt), c["N"] + 1, 2.0), None
    yard = oc.yardstick(oc.ref_linear_dgrad(dt, dy, W, act, saved, d, cdt=torch.float32), r64)
    return r64, oc.measured_bar(r64, yard, dt), yard


def wgrad_bars(dt, c, dy, x, dW0, db0):
    M, N, K = c["M"], c["N"], c["K"]
    acc = c.get("acc", 0)
    dW64, db64 = oc.ref_linear_wgrad(dt, dy, x, dW0 if acc else None, db0 if acc else None)
    kW, kb = M + oc.wgrad_launch(M, N, K)[1], M + oc.colsum_chunks(M)
    bW = kW * oc.U32 * (dy.abs().double().t() @ oc.rnd(x, dt).abs().double() + (dW0.abs().double() if acc else 0))
    bb = kb * oc.U32 * (dy.abs().double().sum(0) + (db0.abs().double() if acc else 0))
    return dW64, db64, bW, bb


def ln_inputs(dt, c, special=False):
    """z rows: unit scale with an offset; every fourth of variance ~1e-3 (a wrong epsilon is a 1 % effect there); one constant
    row.  special: also one row 1000 +- 1 (bf16: 100 +- 1), which a one-pass variance loses"""
    M, E = c["M"], c["E"]
    z = oc.randn((M, E), 21) * 2 + 0.3
    small = torch.arange(M) % 4 == 1
    z[small] = 0.5 + 0.0316 * oc.randn((M, E), 22)[small]
    if M >= 3:
        z[M - 1] = 0.75 if E & (E - 1) == 0 else 0.0      # E * c and 1 / E exact in fp32: the mean is exact, y = beta exactly
    if special:
        # a non-zero constant row at an E that is no power of two: the mean carries one fp32 rounding, rstd = 316 multiplies it.
        # Kept to the `special` cases because that row's yardstick (1e-4 of |beta|) is the worst of its case
        z[M - 3] = 0.75
        z[M - 2] = (100.0 if dt == "bf16" else 1000.0) + torch.sign(oc.randn((E,), 23))     # 1000 +- 1 is no bf16 value
    return (oc.rnd(z, dt), 1 + 0.2 * oc.randn((E,), 24), 0.1 * oc.randn((E,), 25), oc.randn((M, E), 26, dt=dt))


def ln_fwd_bars(dt, z, gamma, beta, pos_rows=None):
    y64, m64, r64 = oc.ref_ln_fwd(z, gamma, beta, pos_rows)
    y32, m32, r32 = oc.ref_ln_fwd(z, gamma, beta, pos_rows, cdt=torch.float32)
    zs = z.double().abs().amax(-1).clamp_min(1e-300)
    yards = {"y": oc.yardstick(y32, y64), "mean": max(float(((m32.double() - m64).abs() / zs).max()), oc.U32),
             "rstd": max(float(((r32.double() - r64).abs() / r64).max()), oc.U32)}
    # y inherits the mean's error times rstd * gamma: one fp32 rounding of the mean (2^-24 of the row's max |z|, the least any
    # fp32 summation promises) is a floor under the yardstick of that row, with the same factor 4
    ys = y64.abs().amax(-1)
    floor = oc.U32 * (ys + r64 * float(gamma.abs().max()) * zs)
    floor = torch.where(r64 > 8, floor, torch.zeros_like(floor))     # low-variance rows only (variance below 1/64): elsewhere
                                                                     # the bar is 4 x the measured yardstick and nothing else
    bar_y = oc.half_ulp(y64, dt) + 4 * torch.maximum(yards["y"] * ys, floor)[:, None]
    yards["floor_rows"] = floor > yards["y"] * ys                  # the rows whose bar is the floor
    bars = {"y": bar_y, "mean": (4 * yards["mean"] * zs)[:, None],
            "rstd": (4 * yards["rstd"] * r64)[:, None]}
    return (y64, m64, r64), bars, yards


def ln_bwd_bars(dt, dy, z, gamma, mean, rstd, dg0=None, db0=None):
    r64 = list(oc.ref_ln_bwd(dy, z, gamma, mean, rstd))
    r32 = list(oc.ref_ln_bwd(dy, z, gamma, mean, rstd, cdt=torch.float32))
    for i, p in ((1, dg0), (2, db0)):
        if p is not None:
            r64[i], r32[i] = r64[i] + p.double(), r32[i] + p
    yards = {k: oc.yardstick(a, b) for k, a, b in zip(("dz", "dgamma", "dbeta"), r32, r64)}
    bars = {"dz": oc.measured_bar(r64[0], yards["dz"], dt), "dgamma": oc.measured_bar(r64[1], yards["dgamma"], "f32"),
            "dbeta": oc.measured_bar(r64[2], yards["dbeta"], "f32")}
    return r64, bars, yards


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests: references, restatements, yardsticks, coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_references_match_autograd():
    """the fp64 references against torch autograd in fp64 (fp32 mode: nothing rounded)"""
    import torch.nn.functional as F
    M, N, K = 9, 7, 11
    x, W, b, r = (oc.randn(s, i).double() for i, s in enumerate([(M, K), (N, K), (N,), (M, N)]))
    dy, d = oc.randn((M, N), 9).double(), oc.randn((M, K), 8).double()
    for act, f in enumerate([lambda t: t, F.relu, lambda t: F.leaky_relu(t, 0.01), F.gelu]):
        xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
        u = F.linear(xr, Wr, br)
        h = f(u)
        y = h + r
        y.backward(dy)
        y64, u64 = oc.ref_linear_fwd("f32", x, W, b, act, r)
        assert torch.allclose(y64, y.detach(), rtol=1e-13, atol=1e-13) and torch.allclose(u64, u.detach(), rtol=1e-13, atol=1e-13)
        saved = u.detach() if act == 3 else h.detach()
        assert torch.allclose(oc.ref_linear_dgrad("f32", dy * oc.act_d(act, saved), W, 0, None, d), xr.grad + d, rtol=1e-12, atol=1e-12)
        du = dy * oc.act_d(act, saved)
        dW, db = oc.ref_linear_wgrad("f32", du, x, W, b)
        assert torch.allclose(dW, Wr.grad + W, rtol=1e-12, atol=1e-12) and torch.allclose(db, br.grad + b, rtol=1e-12, atol=1e-12)
    E = 13
    z, g, be, p = (oc.randn(s, 20 + i).double() for i, s in enumerate([(M, E), (E,), (E,), (M, E)]))
    dy = oc.randn((M, E), 30).double()
    zr, gr, br = (t.clone().requires_grad_(True) for t in (z, g, be))
    (F.layer_norm(zr, (E,), gr, br, 1e-5) + p).backward(dy)
    y64, mu, rs = oc.ref_ln_fwd(z, g, be, p)
    assert torch.allclose(y64, F.layer_norm(z, (E,), g, be, 1e-5) + p, rtol=1e-12, atol=1e-12)
    dz, dg, db = oc.ref_ln_bwd(dy, z, g, mu, rs)
    for a, b_ in ((dz, zr.grad), (dg, gr.grad), (db, br.grad)):
        assert torch.allclose(a, b_, rtol=1e-11, atol=1e-11)
    # the zeros of `saved` take the negative branch, both signs
    s0 = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=torch.float64)
    assert oc.act_d(1, s0).tolist() == [0, 0, 1, 0] and oc.act_d(2, s0).tolist() == [0.01, 0.01, 1, 0.01]


def test_half_ulp():
    assert float(oc.half_ulp(torch.tensor([1.0, 1.99, 2.0, 1e-30]).double(), "bf16")[0]) == 2.0 ** -8
    assert oc.half_ulp(torch.tensor([1.99, 2.0, 1e-9]).double(), "f16").tolist() == [2.0 ** -11, 2.0 ** -10, 2.0 ** -25]
    assert oc.half_ulp(torch.tensor([3.0]).double(), "f32").tolist() == [0.0]


def test_fp32_restatements_and_yardsticks():
    """the fp32 restatements against the references on the accuracy tests' own inputs: prints the yardsticks; they are fp32-sized
    (a restatement that dropped a rounding point, or a reference that added one, is orders of magnitude away)"""
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for dt in ALL:
        for c in oc.LIN_FWD_RANDOM:
            if dt in oc.case_dts(c) and c.get("act") == 3:
                note(("gelu fwd", dt), fwd_bars(dt, c, *fwd_random_operands(dt, c))[4])
        for c in oc.LIN_DGRAD_RANDOM:
            if c.get("act") == 3:
                note(("gelu dgrad", dt), dgrad_bars(dt, c, *dgrad_random_operands(dt, c))[2])
        for c in oc.LN_CASES + oc.LN_MAPS[:2]:
            if c["M"] > 5000:
                continue
            z, g, b, dy = ln_inputs(dt, c, c.get("special", False))
            (_, m64, r64), _, yards = ln_fwd_bars(dt, z, g, b)
            # the floor under LayerNorm's y bar is the bar of low-variance rows only (rstd > 8), never of all rows of a case
            fr = yards.pop("floor_rows")
            assert not bool((fr & (r64 <= 8)).any()) and (c["M"] < 8 or c["E"] == 1 or int(fr.sum()) <= c["M"] // 2), (dt, c["id"])
            _, _, yb = ln_bwd_bars(dt, dy, z, g, m64.float(), r64.float())
            for k, v in {**yards, **yb}.items():
                note(("ln " + k + (" (1000 +- 1 row)" if c.get("special") else ""), dt), v)
    for (k, dt), v in sorted(worst.items()):
        print(f"[operators] yardstick {k:28s} {dt:4s} {v:.3e}")
        assert oc.U32 <= v < (2e-3 if "1000" in k else 2e-5), (k, dt, v)


def test_dispatch_restatements():
    assert oc.fwd_tile("bf16", False, 7, 1, 128) == "64x64" and oc.fwd_tile("f32", False, 65, 130, 33) == "64x64"
    assert oc.fwd_tile("bf16", False, 1000, 1024, 64) == "128x128" and oc.fwd_tile("f32", False, 1000, 1024, 64) == "128x128"
    assert oc.fwd_tile("bf16", True, 24449, 128, 1024) == "64x128" and oc.fwd_tile("bf16", True, 24448, 128, 1024) == "64x64-f32rows"
    assert oc.fwd_tile("f32", True, 24449, 128, 1024) == "128x128"            # fp32 mode never streams
    assert oc.fwd_tile("f16", True, 24449, 128, 1023) == "64x64-f32rows" and oc.fwd_tile("f16", True, 50000, 127, 1024) == "64x64-f32rows"
    assert oc.gemm_tile(2, 2, 4, True, 65, 8193, 8) == "128x128" and oc.gemm_tile(2, 2, 4, True, 64, 8193, 8) == "64x64"
    assert [oc.wgrad_splits(M, 128, 128) for M in (1, 256, 257, 1000, 10 ** 6)] == [1, 1, 2, 4, 384]
    assert oc.wgrad_splits(10 ** 6, 8, 5) == 384 and oc.wgrad_splits(10 ** 6, 2560, 2560) == 1
    assert oc.wgrad_launch(1000, 40, 81) == (256, 4) and oc.wgrad_launch(8200, 8, 5) == (256, 33) and oc.wgrad_launch(200, 40, 81) == (256, 1)
    assert [oc.colsum_chunks(M) for M in (1, 256, 257, 1000, 8191, 8192, 8200, 10 ** 6)] == [1, 1, 5, 16, 128, 16, 17, 256]
    assert oc.wgrad_ws_bytes(200, 40, 81) == 256 and oc.wgrad_ws_bytes(1000, 40, 81) == (4 * 40 * 81 * 4 + 16 * 40 * 4 + 255) // 256 * 256
    assert oc.vec_plan(4, 4, (4, 4), (0, 0)) == (True, 1, 1) and oc.vec_plan(2, 8, (8, 8), (0, 0)) == (True, 1, 1)
    assert oc.vec_plan(4, 96, (96, 96), (0, 0)) == (True, 1, 32) and oc.vec_plan(2, 40, (40, 40), (0, 0)) == (True, 1, 8)
    assert oc.vec_plan(4, 1000, (1000, 1000), (0, 0)) == (True, 4, 64) and oc.vec_plan(2, 1016, (1016, 1016), (0, 0)) == (True, 2, 64)
    assert oc.vec_plan(4, 1024, (1024, 1024), (0, 0)) == (True, 4, 64) and oc.vec_plan(2, 1024, (1024, 1024), (0, 0)) == (True, 2, 64)
    assert not oc.vec_plan(2, 64, (65, 64), (0, 0))[0] and not oc.vec_plan(2, 64, (64, 64), (0, 1))[0] and not oc.vec_plan(4, 66, (68, 68), (0, 0))[0]
    assert [oc.ln_blocks(M) for M in (1, 16, 17, 40001)] == [1, 1, 2, 2048]
    assert [oc.ln_epl(E) for E in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert oc.ln_bwd_ws_bytes(1000, 8) == 3 * 63 * 8 * 4 // 256 * 256 + 256
    assert oc.map_rows(6, (2, 3, 1)).tolist() == [1, 2, 3, 5, 6, 7]


def _reached(cases, fn):
    seen = {}
    for c in cases:
        for dt in oc.case_dts(c):
            for k, v in fn(c, dt).items():
                seen.setdefault((k, dt == "f32"), set()).add(v)
    return seen


def test_linear_cases_cover_every_branch():
    """trimming a case list fails here.  Keys: (what, fp32 mode?)"""
    stage = {"vector", "vector-tail", "scalar-stride", "scalar-pointer"}
    store16 = {"vector", "vector+scalar-tail", "scalar-ldc", "scalar-c-pointer", "scalar-other-stride", "scalar-other-pointer"}
    f = _reached(oc.LIN_FWD + oc.LIN_FWD_FUSIONS, oc.lin_fwd_branches)
    assert f[("tile", True)] == {"64x64", "128x128"}
    assert f[("tile", False)] == {"64x64", "128x128", "64x128", "64x64-f32rows"}
    assert f[("stage_x", True)] == stage and f[("stage_x", False)] == stage and f[("store", False)] == store16
    assert f[("k_tiles", True)] == {"one", "many"} and f[("k_tiles", False)] == {"one", "many"}
    fus = {(c.get("act", 0), bool(c.get("ldr")), bool(c.get("pre"))) for c in oc.LIN_FWD_FUSIONS}
    assert fus == {(a, r, p) for a in range(4) for r in (False, True) for p in (False, True)}
    assert fus <= {(c.get("act", 0), bool(c.get("ldr")), bool(c.get("pre"))) for c in oc.LIN_FWD_RANDOM}
    # the streamed fp32 rows below and above the 64x128 threshold, and that threshold is the smallest M
    big = [c for c in oc.LIN_FWD if c["id"] == "xf32-t64x128"][0]
    assert oc.fwd_tile("bf16", True, big["M"] - 1, big["N"], big["K"]) == "64x64-f32rows"
    d = _reached(oc.LIN_DGRAD + oc.LIN_DGRAD_FUSIONS, oc.lin_dgrad_branches)
    assert d[("tile", True)] == {"64x64", "128x128"} and d[("tile", False)] == {"64x64", "128x128"}
    assert d[("stage_dy", True)] == stage and d[("stage_dy", False)] == stage and d[("store", False)] == store16
    dfus = {(c.get("act", 0), bool(c.get("lddr"))) for c in oc.LIN_DGRAD_FUSIONS}
    assert dfus == {(a, r) for a in range(4) for r in (False, True)}
    assert dfus <= {(c.get("act", 0), bool(c.get("lddr"))) for c in oc.LIN_DGRAD_RANDOM}
    # saved / dres strides and pointers each take the scalar epilogue once
    ids = {c["id"] for c in oc.LIN_DGRAD}
    assert {"store-lds43", "store-lddr43", "store-saved-ptr", "store-dres-ptr"} <= ids
    w = _reached(oc.LIN_WGRAD, oc.lin_wgrad_branches)
    for f32 in (True, False):
        assert w[("tile", f32)] == {"64x64", "128x128"}
        assert w[("dW", f32)] == {"in-kernel", "in-kernel-acc", "slabs", "slabs-acc"}
        assert w[("db", f32)] == {"one-chunk-direct", "one-chunk-reduce", "chunks-of-64", "chunks-of-512"}
        assert w[("stage_dy", f32)] == stage
    assert w[("stage_x", True)] == stage and w[("stage_x", False)] == stage
    for s in oc._WG_SHAPES:                                  # every reduction regime with every output combination
        got = {(c.get("acc", 0), c.get("dW", True), c.get("db", True)) for c in oc.LIN_WGRAD if c["id"].startswith(s["id"])}
        assert got >= {(0, True, True), (1, True, True), (0, True, False), (0, False, True), (1, False, True)}
    assert any(c.get("xf32") and oc.stage_branch(4, c.get("ldx", c["K"]), c["K"], 0) == "vector-tail" for c in oc.LIN_WGRAD)
    assert any(c.get("xf32") and oc.stage_branch(4, c.get("ldx", c["K"]), c["K"], 0) == "vector-tail" for c in oc.LIN_FWD)


def test_layernorm_cases_cover_every_branch():
    fwd, bwd, reasons = {}, {}, {}
    for c in oc.LN_CASES + oc.LN_MAPS:
        for dt in ALL:
            a = (c["E"], c["ldz"], c["ldy"], c.get("zo", 0), c.get("yo", 0), c["M"])
            if c.get("fwd", True):
                k = oc.ln_fwd_branch(dt, *a)
                fwd.setdefault(dt, set()).add(k[:3] + (k[3] > 1,))
            if c.get("bwd", True):
                k = oc.ln_bwd_branch(dt, c["E"], c["ldy"], c["ldz"], c["lddz"], c.get("yo", 0), c.get("zo", 0), c.get("dzo", 0), c["M"])
                bwd.setdefault(dt, set()).add(k[:3] + (k[3] > 0,))
            reasons.setdefault(dt, set()).add(oc.ln_fallback_reason(dt, c["E"], c["ldz"], c["ldy"], c["lddz"], c.get("zo", 0), c.get("yo", 0)))
    for dt in ALL:
        V = 16 // ESIZE[dt]
        for kind, seen in (("fwd", fwd[dt]), ("bwd", bwd[dt])):
            assert {k[1] for k in seen if k[0] == "scalar"} == {1, 2, 4, 8, 16}, (dt, kind)           # every EPL
            assert {k[1] for k in seen if k[0] == "vec"} == ({1, 2, 4} if V == 4 else {1, 2}), (dt, kind)
            assert {1, 64} <= {k[2] for k in seen if k[0] == "vec"}, (dt, kind)                       # one lane per row .. a whole wave
        assert any(k[3] for k in fwd[dt] if k[0] == "vec") and any(k[3] for k in fwd[dt] if k[0] == "scalar")   # grid-stride loops
        assert any(k[3] for k in bwd[dt] if k[0] == "vec")                                            # blocks that own no row
        assert reasons[dt] >= {"ldz", "ldy", "pointer", "lddz"}
        # lanes per row that are not all used, and a partly empty last lane at NV > 1
        needs = {(c["E"] // V) for c in oc.LN_CASES if c["E"] % V == 0}
        assert any(n & (n - 1) for n in needs if n <= 64) and any(n > 64 and n % (2 if n <= 128 else 4) for n in needs)
    assert {e for e, _ in oc.LN_SCALAR_E} == {1, 33, 64, 65, 129, 257, 513, 1023}
    assert {(c["mp"], c.get("pos")) for c in oc.LN_MAPS} >= {((B, T, off), p) for B in (1, 3) for T in (1, 7) for off in (0, 1)
                                                             for p in (False, True)}
    acc = {(c.get("acc", 0), c.get("dgamma", True), c.get("dbeta", True)) for c in oc.LN_CASES}
    assert acc >= {(a, g, b) for a in (0, 1) for g, b in ((True, True), (True, False), (False, True))}
    assert any(c["M"] == 1 for c in oc.LN_CASES)


@pytest.mark.parametrize("dt,c", _params(oc.LIN_FWD + oc.LIN_FWD_FUSIONS))
def test_integer_cases_are_exactly_representable_fwd(dt, c):
    x, W, b, r = fwd_int_operands(c)
    y64, u64 = oc.ref_linear_fwd(dt, x, W, b, c.get("act", 0) if c.get("act", 0) <= 1 else 0, r if c.get("ldr") else None)
    assert float(y64.abs().max()) <= INT_LIMIT[dt] and float(u64.abs().max()) <= INT_LIMIT[dt]
    if c["M"] * c["N"] >= 64:
        assert float(y64.abs().max()) > 8 and len(torch.unique(y64)) > 8      # not a degenerate pattern


def test_integer_cases_are_exactly_representable_bwd():
    for c in oc.LIN_DGRAD + oc.LIN_DGRAD_FUSIONS:
        dy, W, s, d = dgrad_int_operands(c)
        r = oc.ref_linear_dgrad("f32", dy, W, min(c.get("act", 0), 1), s, d if c.get("lddr") else None)
        assert float(r.abs().max()) <= 256 and len(torch.unique(r)) > 2
        if c["M"] * c["K"] >= 25:                                # saved holds +0.0 and -0.0
            assert bool(((s == 0) & ~torch.signbit(s)).any()) and bool(((s == 0) & torch.signbit(s)).any())
    for c in oc.LIN_WGRAD:
        dy, x, dW0, db0 = wgrad_int_operands(c)
        dW, db = oc.ref_linear_wgrad("f32", dy, x, dW0, db0)
        assert float(dW.abs().max()) < 2 ** 24 and float(db.abs().max()) < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------
# GPU: linear, exact
# ---------------------------------------------------------------------------------------------------------------------
def _equal(got, ref64, dt, what):
    want = ref64.to(DT[dt])
    assert bool((want.double() == ref64).all()), "the test's own operands are not exact in " + dt
    bad = (got.float() != want.float())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} mismatches, first at {bad.nonzero()[0].tolist()}"


@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LIN_FWD + oc.LIN_FWD_FUSIONS))
def test_linear_fwd_exact(dt, c):
    """integers: y_preact exact under every act, y exact for none / relu; leaky and gelu against their bars"""
    x, W, b, r = fwd_int_operands(c)
    y, pre = run_fwd(dt, c, x, W, b, r)
    y64, u64 = oc.ref_linear_fwd(dt, x, W, b, c.get("act", 0), r if c.get("ldr") else None)
    if pre is not None:
        _equal(pre, u64, dt, "y_preact")
    if c.get("act", 0) <= 1:
        _equal(y, y64, dt, "y")
    else:
        _check("linear_fwd", dt, c["id"] + " (integers)", y, y64, fwd_bars(dt, c, x, W, b, r)[2])


@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LIN_DGRAD + oc.LIN_DGRAD_FUSIONS))
def test_linear_dgrad_exact(dt, c):
    dy, W, s, d = dgrad_int_operands(c)
    dx = run_dgrad(dt, c, dy, W, s, d)
    r64, bar, _ = dgrad_bars(dt, c, dy, W, s, d)
    if c.get("act", 0) <= 1:
        _equal(dx, r64, dt, "dx")
    else:
        _check("linear_dgrad", dt, c["id"] + " (integers)", dx, r64, bar)


@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LIN_WGRAD))
def test_linear_wgrad_exact(dt, c):
    """out == prefill + reference exactly on every reduction branch; a NULL output leaves nothing behind"""
    dy, x, dW0, db0 = wgrad_int_operands(c)
    dW, db = run_wgrad(dt, c, dy, x, dW0, db0)
    acc = c.get("acc", 0)
    dW64, db64 = oc.ref_linear_wgrad(dt, dy, x, dW0 if acc else None, db0 if acc else None)
    if dW is not None:
        _equal(dW, dW64, "f32", "dW")
    if db is not None:
        _equal(db, db64, "f32", "db")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: linear, accuracy
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LIN_FWD_RANDOM))
def test_linear_fwd_accuracy(dt, c):
    ops = fwd_random_operands(dt, c)
    y, pre = run_fwd(dt, c, *ops)
    y64, u64, bar_y, bar_u, _ = fwd_bars(dt, c, *ops)
    if pre is not None:
        _check("linear_fwd", dt, c["id"] + " y_preact", pre, u64, bar_u)
    _check("linear_fwd", dt, c["id"] + " y", y, y64, bar_y)


@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LIN_DGRAD_RANDOM))
def test_linear_dgrad_accuracy(dt, c):
    ops = dgrad_random_operands(dt, c)
    dx = run_dgrad(dt, c, *ops)
    r64, bar, _ = dgrad_bars(dt, c, *ops)
    _check("linear_dgrad", dt, c["id"], dx, r64, bar)


@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LIN_WGRAD_RANDOM))
def test_linear_wgrad_accuracy(dt, c):
    ops = wgrad_random_operands(dt, c)
    dW, db = run_wgrad(dt, c, *ops)
    dW64, db64, bW, bb = wgrad_bars(dt, c, *ops)
    _check("linear_wgrad", dt, c["id"] + " dW", dW, dW64, bW)
    _check("linear_wgrad", dt, c["id"] + " db", db, db64, bb)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(ITYPE[t.element_size()])


@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LN_CASES))
def test_layernorm_accuracy(dt, c):
    z, g, b, dy = ln_inputs(dt, c, c.get("special", False))
    (y64, m64, r64), bars, _ = ln_fwd_bars(dt, z, g, b)
    if c.get("fwd", True):
        y, mean, rstd = run_ln_fwd(dt, c, z, g, b)
        _check("layernorm_fwd", dt, c["id"] + " y", y, y64, bars["y"])
        _check("layernorm_fwd", dt, c["id"] + " mean", mean[:, None], m64[:, None], bars["mean"])
        _check("layernorm_fwd", dt, c["id"] + " rstd", rstd[:, None], r64[:, None], bars["rstd"])
        if c["M"] >= 3:     # the constant row: rstd = 1 / sqrt(1e-5), y = beta
            assert abs(float(rstd[-1]) * 1e-5 ** 0.5 - 1) < 1e-6
            if c["E"] & (c["E"] - 1) == 0:
                assert torch.equal(y[-1].float(), b.to(DT[dt]).float())
    if c.get("bwd", True):
        acc = c.get("acc", 0)
        dg0, db0 = (oc.randn((c["E"],), 31), oc.randn((c["E"],), 32)) if acc else (None, None)
        mean, rstd = m64.float(), r64.float()
        dz, dg, db = run_ln_bwd(dt, c, dy, z, g, mean, rstd, dg0, db0)
        r, bb, _ = ln_bwd_bars(dt, dy, z, g, mean, rstd, dg0, db0)
        _check("layernorm_bwd", dt, c["id"] + " dz", dz, r[0], bb["dz"])
        if dg is not None:
            _check("layernorm_bwd", dt, c["id"] + " dgamma", dg, r[1], bb["dgamma"])
        if db is not None:
            _check("layernorm_bwd", dt, c["id"] + " dbeta", db, r[2], bb["dbeta"])


@gpu
@pytest.mark.parametrize("dt,c", _params(oc.LN_MAPS))
def test_layernorm_row_map_and_pos(dt, c):
    """token assembly behind the regression token: placement is exact"""
    M, E, (B, T, off) = c["M"], c["E"], c["mp"]
    S = T + off
    z, g, b, dy = ln_inputs(dt, c)
    rows = oc.map_rows(M, c["mp"])
    plain = dict(c, mp=None)
    assert oc.ln_fwd_branch(dt, E, c["ldz"], c["ldy"], 0, 0, M)[:3] == oc.ln_fwd_branch(dt, E, plain["ldz"], plain["ldy"], 0, 0, M)[:3]
    y_u, mean_u, rstd_u = run_ln_fwd(dt, plain, z, g, b)
    y_m, mean_m, rstd_m = run_ln_fwd(dt, c, z, g, b)
    assert torch.equal(_bits(y_m), _bits(y_u)) and torch.equal(_bits(mean_m), _bits(mean_u)) and torch.equal(_bits(rstd_m), _bits(rstd_u))
    (y64, m64, r64), bars, _ = ln_fwd_bars(dt, z, g, b)
    _check("layernorm_fwd", dt, c["id"] + " y", y_m, y64, bars["y"])
    if c.get("pos"):
        # pos is indexed by the position in the OUTPUT sequence, offset included: rows below `off` are never read (NaN)
        pos = oc.randn((S, E), 41)
        pos[:off] = float("nan")
        pos_rows = pos[rows % S]
        y_p, _, _ = run_ln_fwd(dt, c, z, g, b, pos)
        (yp64, _, _), pbars, _ = ln_fwd_bars(dt, z, g, b, pos_rows)
        _check("layernorm_fwd", dt, c["id"] + " y+pos", y_p, yp64, pbars["y"])
        if dt == "f32":
            assert torch.equal(_bits(y_p), _bits(y_m + pos_rows))            # one IEEE add on top of the stored value
        # exact in every dtype: gamma = 0 leaves beta + pos, small integers plus signed powers of two distinct per position
        beta_i = oc.ints((E,), 3, 0, 7, -3)
        pos_i = (2.0 ** ((torch.arange(S)[:, None] + torch.arange(E)[None, :]) % 6)) * (1 - 2 * (torch.arange(S)[:, None] % 2))
        pos_i[:off] = float("nan")
        y_i, _, _ = run_ln_fwd(dt, c, z, torch.zeros(E), beta_i, pos_i)
        _equal(y_i, (beta_i[None] + pos_i[rows % S]).double(), dt, "beta + pos")
    # the backward reads dy through the same map: bitwise the unmapped pair
    mean, rstd = m64.float(), r64.float()
    out_u = run_ln_bwd(dt, plain, dy, z, g, mean, rstd)
    out_m = run_ln_bwd(dt, c, dy, z, g, mean, rstd)
    for a, b_ in zip(out_m, out_u):
        assert torch.equal(_bits(a), _bits(b_))
    # ... and forward then backward on the mapped buffer itself (dy := y, as a stand-in gradient)
    dz_m = run_ln_bwd(dt, c, y_m.float(), z, g, mean_m, rstd_m)
    dz_u = run_ln_bwd(dt, plain, y_u.float(), z, g, mean_u, rstd_u)
    for a, b_ in zip(dz_m, dz_u):
        assert torch.equal(_bits(a), _bits(b_))
