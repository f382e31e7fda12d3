"""References, dispatch restatements, bars and case lists of tests/test_operators_gpu.py (no GPU needed to import this).

Everything here is plain torch on the CPU.  The references take the compute dtype `cdt`: torch.float64 is the reference,
torch.float32 the restatement whose error against the reference is the yardstick of the bars that have no closed form.
"""
import math

import torch

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}
ESIZE = {"f32": 4, "bf16": 2, "f16": 2}
PREC = {"bf16": 8, "f16": 11}            # significant bits
EMIN = {"bf16": -126, "f16": -14}        # exponent of the smallest normal
ACT_NAMES = {0: "none", 1: "relu", 2: "leaky", 3: "gelu"}
U32 = 2.0 ** -24                          # fp32 unit roundoff
LN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# dispatch restatements (csrc/gemm.hip, csrc/norm.hip)
# ---------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def gemm_tile(t_bytes, ta_bytes, tb_bytes, la_kc, M, N, K, splits=1):
    """launch_gemm_t (gemm.hip:350-372) on the GEMM's own M, N, K: the branch taken"""
    big = cdiv(M, 128) * cdiv(N, 128) * splits
    if ta_bytes == 4 and t_bytes == 2 and la_kc and K >= 1024 and N >= 128 and big >= 192:
        return "64x128"
    if ta_bytes == 4 and t_bytes == 2 and tb_bytes == 4 and la_kc:
        return "64x64-f32rows"
    if big >= 192 or (M > 64 and N > 64 and big >= 64):
        return "128x128"
    return "64x64"


def fwd_tile(dt, x_f32, M, N, K):
    t = ESIZE[dt]
    return gemm_tile(t, 4 if (x_f32 or dt == "f32") else 2, 4, True, M, N, K)


def dgrad_tile(dt, M, N, K):
    """dx[M,K] = dy[M,N] W[N,K]: the GEMM is (M, K, N)"""
    return gemm_tile(ESIZE[dt], ESIZE[dt], 4, True, M, K, N)


def wgrad_splits(M, N, K):
    tiles = cdiv(N, 128) * cdiv(K, 128)
    want = (384 + tiles - 1) // tiles
    maxs = (M + 255) // 256
    return max(1, min(want, maxs, 512))


def wgrad_launch(M, N, K):
    """(k_chunk, splits actually launched) of launch_linear_wgrad"""
    sp = wgrad_splits(M, N, K)
    k_chunk = (cdiv(M, sp) + 63) // 64 * 64
    return k_chunk, cdiv(M, k_chunk)


def wgrad_tile(dt, x_f32, M, N, K):
    """dW[N,K] = dy^T x: the GEMM is (N, K, M), both operands k-strided"""
    return gemm_tile(ESIZE[dt], ESIZE[dt], 4 if (x_f32 or dt == "f32") else 2, False, N, K, M, wgrad_launch(M, N, K)[1])


def colsum_chunks(M):
    if M <= 256:
        return 1
    return max(1, min(256, cdiv(M, 64 if M < 8192 else 512)))


def colsum_regime(M, accumulate):
    c = colsum_chunks(M)
    if c == 1:
        return "one-chunk-reduce" if accumulate else "one-chunk-direct"
    return "chunks-of-64" if M < 8192 else "chunks-of-512"


def wgrad_ws_bytes(M, N, K):
    sp = wgrad_splits(M, N, K)
    b = (sp * N * K * 4 if sp > 1 else 0) + colsum_chunks(M) * N * 4
    return cdiv(b, 256) * 256


def stage_branch(esize, ld, extent, off):
    """which path the staging loads of one operand take along its contiguous extent (StageKC / StageKS::load)"""
    V = 16 // esize
    if ld % V:
        return "scalar-stride"
    if (off * esize) % 16:
        return "scalar-pointer"
    return "vector" if extent % V == 0 else "vector-tail"


def store_branch(dt, ncols, ldc, c_off, others):
    """epilogue of the 16-bit store (gemm.hip:287-343).  `others`: (ld, element offset) of resid / saved / y_preact"""
    if dt == "f32":
        return "fp32"
    if ldc % 8:
        return "scalar-ldc"
    if (c_off * 2) % 16:
        return "scalar-c-pointer"
    for ld, off in others:
        if ld % 8:
            return "scalar-other-stride"
        if (off * 2) % 16:
            return "scalar-other-pointer"
    return "vector" if ncols % 8 == 0 else "vector+scalar-tail"


def vec_plan(esize, E, lds, offs):
    """vec_plan (norm.hip:295-312): (ok, NV, LPR).  lds: the strides checked, offs: element offsets of the pointers"""
    V = 16 // esize
    if E % V or any(ld % V for ld in lds):
        return (False, 1, 64)
    if any((o * esize) % 16 for o in offs):
        return (False, 1, 64)
    vecs = E // V
    nv = 1 if vecs <= 64 else (2 if vecs <= 128 else 4)
    if vecs > 256:
        return (False, nv, 64)
    need = cdiv(vecs, nv)
    lpr = 1
    while lpr < need:
        lpr <<= 1
    return (True, nv, lpr)


def ln_blocks(M):
    return max(1, min(2048, cdiv(M, 16)))


def ln_epl(E):
    return 1 if E <= 64 else 2 if E <= 128 else 4 if E <= 256 else 8 if E <= 512 else 16


def ln_bwd_ws_bytes(M, E):
    return cdiv(3 * ln_blocks(M) * E * 4, 256) * 256


def ln_fwd_branch(dt, E, ldz, ldy, zoff, yoff, M):
    """(kernel, parameters, sweeps of the grid-stride loop)"""
    ok, nv, lpr = vec_plan(ESIZE[dt], E, (ldz, ldy), (zoff, yoff))
    if ok:
        rpb = 4 * (64 // lpr)
        blocks = min(2048, cdiv(M, rpb))
        return ("vec", nv, lpr, cdiv(M, blocks * rpb))
    return ("scalar", ln_epl(E), 64, cdiv(M, ln_blocks(M) * 4))


def ln_bwd_branch(dt, E, lddy, ldz, lddz, dyoff, zoff, dzoff, M):
    ok, nv, lpr = vec_plan(ESIZE[dt], E, (lddy, ldz), (dyoff, zoff, dzoff))
    if ok and lddz % (16 // ESIZE[dt]) == 0:
        rows_per_block = 4 * (64 // lpr)
        return ("vec", nv, lpr, ln_blocks(M) - cdiv(M, rows_per_block))     # last: blocks that own no row
    return ("scalar", ln_epl(E), 64, 0)


def ln_fallback_reason(dt, E, ldz, ldy, lddz, zoff, yoff):
    V = 16 // ESIZE[dt]
    if E % V or E // V > 256:
        return None
    if ldz % V:
        return "ldz"
    if ldy % V:
        return "ldy"
    if (zoff * ESIZE[dt]) % 16 or (yoff * ESIZE[dt]) % 16:
        return "pointer"
    if lddz % V:
        return "lddz"
    return None


def map_rows(M, mp):
    """output row of every input row: mp = (B, T, off) -> (r // T) * (T + off) + r % T + off"""
    r = torch.arange(M)
    if mp is None:
        return r
    B, T, off = mp
    assert B * T == M
    return (r // T) * (T + off) + r % T + off


# ---------------------------------------------------------------------------------------------------------------------
# references: cdt = float64 the reference, float32 the restatement.  All return UNROUNDED final values in cdt; `rnd`
# applies the one final rounding of the kernel.
# ---------------------------------------------------------------------------------------------------------------------
def rnd(x, dt):
    return x if dt == "f32" else x.to(DT[dt]).to(x.dtype)


def act_f(act, u):
    if act == 1:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == 2:
        return torch.where(u > 0, u, 0.01 * u)
    if act == 3:
        return 0.5 * u * (1 + torch.erf(u * 0.70710678118654752))
    return u


def act_d(act, s):
    """common.h:80-90: `s > 0` strict, so 0 and -0.0 take the negative branch"""
    if act == 1:
        return (s > 0).to(s.dtype)
    if act == 2:
        return torch.where(s > 0, torch.ones_like(s), torch.full_like(s, 0.01))
    if act == 3:
        return 0.5 * (1 + torch.erf(s * 0.70710678118654752)) + s * 0.3989422804014327 * torch.exp(-0.5 * s * s)
    return torch.ones_like(s)


def ref_linear_fwd(dt, x, W, bias, act, resid, cdt=torch.float64):
    """x, W, bias, resid: fp32 tensors holding what the caller passes.  -> (y, y_preact), unrounded"""
    u = rnd(x, dt).to(cdt) @ rnd(W, dt).to(cdt).t()
    if bias is not None:
        u = u + bias.to(cdt)
    y = act_f(act, u)
    if resid is not None:
        y = y + resid.to(cdt)
    return y, u


def ref_linear_dgrad(dt, dy, W, act, saved, dres, cdt=torch.float64):
    v = dy.to(cdt) @ rnd(W, dt).to(cdt)
    if act:
        v = v * act_d(act, saved.to(cdt))
    if dres is not None:
        v = v + dres.to(cdt)
    return v


def ref_linear_wgrad(dt, dy, x, dW0=None, db0=None, cdt=torch.float64):
    dW = dy.to(cdt).t() @ rnd(x, dt).to(cdt)
    db = dy.to(cdt).sum(0)
    if dW0 is not None:
        dW = dW + dW0.to(cdt)
    if db0 is not None:
        db = db + db0.to(cdt)
    return dW, db


def ref_ln_fwd(z, gamma, beta, pos_rows=None, cdt=torch.float64):
    """pos_rows: pos already gathered per input row, [M,E].  -> (y unrounded, mean, rstd)"""
    z = z.to(cdt)
    inv = torch.ones((), dtype=cdt) / z.shape[-1]                  # the kernels multiply by invE = 1.f / E
    mu = z.sum(-1, keepdim=True) * inv
    var = ((z - mu) ** 2).sum(-1, keepdim=True) * inv
    rs = torch.rsqrt(var + LN_EPS)
    y = (z - mu) * rs * gamma.to(cdt) + beta.to(cdt)
    if pos_rows is not None:
        y = y + pos_rows.to(cdt)
    return y, mu.squeeze(-1), rs.squeeze(-1)


def ref_ln_bwd(dy, z, gamma, mean, rstd, cdt=torch.float64):
    """mean / rstd are inputs (the kernel is given the same ones).  -> (dz unrounded, dgamma, dbeta)"""
    dy, z = dy.to(cdt), z.to(cdt)
    xh = (z - mean.to(cdt)[:, None]) * rstd.to(cdt)[:, None]
    g = dy * gamma.to(cdt)
    inv = torch.ones((), dtype=cdt) / z.shape[-1]
    s1 = g.sum(-1, keepdim=True) * inv
    s2 = (g * xh).sum(-1, keepdim=True) * inv
    dz = rstd.to(cdt)[:, None] * (g - s1 - xh * s2)
    return dz, (dy * xh).sum(0), dy.sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------
def half_ulp(ref, dt):
    """half an ulp of the element type at every element of `ref` (0 for fp32 outputs): 2^(floor(log2|x|) - p), which is
    between 2^-(p+1) and 2^-p of |x| -- 2^-9 .. 2^-8 in bf16, 2^-12 .. 2^-11 in fp16 -- and 2^(emin - p) below the normals"""
    if dt == "f32":
        return torch.zeros_like(ref)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** (EMIN[dt] - 1)))).clamp_min(EMIN[dt])
    return torch.pow(2.0, e - PREC[dt])


def gemm_fp32_term(A, B, k_red, factor=1.0):
    """order-independent bound on an fp32 dot product: k_red * 2^-24 * (|A| @ |B|)"""
    return factor * k_red * U32 * (A.abs().double() @ B.abs().double())


def row_ratio(got, ref, bar):
    """worst |got - ref| / bar, element by element (sharper than the row's largest error against the row's largest bar: a
    small element may not be off by half an ulp of a large one).  -> (ratio, error, bar, row) of the worst element.  1-D: one row"""
    got, ref = got.double(), ref.double()
    if got.dim() == 1:
        got, ref, bar = got[None], ref[None], (bar[None] if bar.dim() == 1 else bar)
    err = (got - ref).abs()
    b = bar.double().expand_as(err)
    ratio = torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), float(err.flatten()[i]), float(b.flatten()[i]), i // ratio.shape[-1]


def yardstick(r32, r64):
    """worst per-row error of the fp32 restatement, relative to the row's largest reference magnitude; never below one fp32
    rounding (2^-24: the stored fp32 value itself is rounded once, whatever the summation order)"""
    r32, r64 = r32.double(), r64.double()
    if r64.dim() == 1:
        r32, r64 = r32[None], r64[None]
    scale = r64.abs().amax(-1).clamp_min(1e-300)
    return max(float(((r32 - r64).abs().amax(-1) / scale).max()), U32)


def measured_bar(ref, yard, dt_out):
    """half an ulp + 4 x the yardstick x the row's scale"""
    r = ref.double()
    if r.dim() == 1:
        return half_ulp(r, dt_out) + 4 * yard * r.abs().max()
    return half_ulp(r, dt_out) + 4 * yard * r.abs().amax(-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def ints(shape, a, b, mod, lo, mix=0):
    """asymmetric small-integer pattern ((i * a + j * b + (i * j) % 11 * mix) % mod) + lo as fp32"""
    i = torch.arange(shape[0])[:, None] if len(shape) == 2 else torch.arange(shape[0])
    j = torch.arange(shape[1])[None, :] if len(shape) == 2 else 0
    return ((i * a + j * b + ((i * j) % 11) * mix) % mod + lo).float()


def randn(shape, seed, scale=1.0, dt=None):
    v = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale
    return rnd(v, dt) if dt else v


# ---------------------------------------------------------------------------------------------------------------------
# case lists.  Strides / offsets in elements; None = absent.
# ---------------------------------------------------------------------------------------------------------------------
def _c(**kw):
    return kw


ALL = ("f32", "bf16", "f16")
H16 = ("bf16", "f16")

# forward: x[M,K] ldx, y / y_preact[M,N] ldy, resid ldr.  offsets: xo, yo, ro, po
LIN_FWD = [
    _c(id="t64-7x1x128", M=7, N=1, K=128),
    _c(id="t64-65x130x33", M=65, N=130, K=33, ldr=130, pre=True, act=1),
    _c(id="k-below-tile-1x3x5", M=1, N=3, K=5, ldr=3, pre=True),
    _c(id="ragged-129x130x131", M=129, N=130, K=131, ldr=130, pre=True, act=1),
    _c(id="t128-1000x1024x64", M=1000, N=1024, K=64, ldr=1024, act=1),
    _c(id="tail-ldx88", M=33, N=40, K=81, ldx=88, ldy=40, ldr=40, pre=True),
    _c(id="tail-ldx83", M=33, N=40, K=81, ldx=83, ldy=48, ldr=48),
    _c(id="tail-ldx88-ptr", M=33, N=40, K=81, ldx=88, xo=1, ldy=48, ldr=48),
    _c(id="store-vector", M=70, N=40, K=64, ldy=48, ldr=56, pre=True, act=1),
    _c(id="store-ldy43", M=70, N=40, K=64, ldy=43, ldr=48, pre=True),
    _c(id="store-resid-ptr", M=70, N=40, K=64, ldy=48, ldr=48, ro=1),
    _c(id="store-ldr43", M=70, N=40, K=64, ldy=48, ldr=43, pre=True, act=1),
    _c(id="store-n43", M=70, N=43, K=64, ldy=48, ldr=48, pre=True),
    _c(id="store-y-ptr", M=70, N=40, K=64, ldy=48, yo=1, ldr=48),
    _c(id="store-preact-ptr", M=70, N=40, K=64, ldy=48, ldr=48, pre=True, po=1),
    _c(id="xf32-t64", M=65, N=130, K=33, xf32=True, ldr=130, dts=H16),
    _c(id="xf32-tail-ldx84", M=33, N=40, K=81, ldx=84, xf32=True, ldy=48, ldr=48, pre=True, dts=H16),
    _c(id="xf32-ldx83", M=33, N=40, K=81, ldx=83, xf32=True, ldy=48, dts=H16),
    _c(id="xf32-t64x128", M=24449, N=128, K=1024, xf32=True, ldr=128, dts=H16),
]
# every fusion: act x resid x preact, on a strided shape with a vector tail
LIN_FWD_FUSIONS = [_c(id=f"{ACT_NAMES[a]}-r{int(r)}-p{int(p)}", M=67, N=43, K=81, ldx=88, ldy=48, ldr=(56 if r else None),
                      pre=p, act=a) for a in range(4) for r in (False, True) for p in (False, True)]
LIN_FWD_RANDOM = LIN_FWD_FUSIONS + [
    _c(id="t128", M=300, N=260, K=96, ldr=260, act=3, pre=True),
    _c(id="ragged", M=129, N=130, K=131, ldr=130, act=2),
    _c(id="xf32", M=65, N=130, K=133, xf32=True, ldr=130, act=3, dts=H16),
]

# dgrad: dy[M,N] lddy, W[N,K], saved / dres / dx [M,K] lds / lddr / lddx.  offsets: dyo, so, ro, dxo
LIN_DGRAD = [
    _c(id="t64-7x128x1", M=7, N=128, K=1),
    _c(id="t64-65x33x130", M=65, N=33, K=130, act=1, lds=130, lddr=130),
    _c(id="k-below-tile-1x5x3", M=1, N=5, K=3, act=1, lds=3, lddr=3),
    _c(id="ragged-129x131x130", M=129, N=131, K=130, act=1, lds=130, lddr=130),
    _c(id="t128-1000x64x1024", M=1000, N=64, K=1024, act=1, lds=1024, lddr=1024),
    _c(id="tail-lddy88", M=33, N=81, K=40, lddy=88, lddx=40, act=1, lds=40, lddr=40),
    _c(id="tail-lddy83", M=33, N=81, K=40, lddy=83, lddx=48),
    _c(id="tail-lddy88-ptr", M=33, N=81, K=40, lddy=88, dyo=1, lddx=48),
    _c(id="store-vector", M=70, N=64, K=40, lddx=48, act=1, lds=56, lddr=64),
    _c(id="store-lddx43", M=70, N=64, K=40, lddx=43, act=1, lds=48, lddr=48),
    _c(id="store-lds43", M=70, N=64, K=40, lddx=48, act=1, lds=43, lddr=48),
    _c(id="store-lddr43", M=70, N=64, K=40, lddx=48, act=1, lds=48, lddr=43),
    _c(id="store-saved-ptr", M=70, N=64, K=40, lddx=48, act=1, lds=48, so=1, lddr=48),
    _c(id="store-dres-ptr", M=70, N=64, K=40, lddx=48, act=1, lds=48, lddr=48, ro=1),
    _c(id="store-k43", M=70, N=64, K=43, lddx=48, act=1, lds=56, lddr=48),
    _c(id="store-dx-ptr", M=70, N=64, K=40, lddx=48, dxo=1, act=1, lds=48),
]
LIN_DGRAD_FUSIONS = [_c(id=f"{ACT_NAMES[a]}-d{int(d)}", M=67, N=81, K=43, lddy=88, lddx=48, act=a, lds=(56 if a else None),
                        lddr=(64 if d else None)) for a in range(4) for d in (False, True)]
LIN_DGRAD_RANDOM = LIN_DGRAD_FUSIONS + [
    _c(id="t128", M=300, N=96, K=260, act=3, lds=260, lddr=260),
    _c(id="ragged", M=129, N=131, K=130, act=2, lds=130),
]

# wgrad: dy[M,N] lddy, x[M,K] ldx -> dW[N,K], db[N].  offsets: dyo, xo
_WG_SHAPES = [
    _c(id="one-split-200x40x81", M=200, N=40, K=81),
    _c(id="splits-1000x40x81", M=1000, N=40, K=81),
    _c(id="t128-4200x130x130", M=4200, N=130, K=130),
    _c(id="chunks512-8200x8x5", M=8200, N=8, K=5),
]
_WG_VARIANTS = [("", {}), ("-acc", dict(acc=1)), ("-nodb", dict(db=False)), ("-nodW", dict(dW=False)),
                ("-acc-nodW", dict(acc=1, dW=False))]
LIN_WGRAD = [dict(s, id=s["id"] + n, **v) for s in _WG_SHAPES for n, v in _WG_VARIANTS] + [
    _c(id="k-below-tile-5x3x1", M=5, N=3, K=1),
    _c(id="vector-200x40x64", M=200, N=40, K=64),
    _c(id="tail-88-88", M=200, N=81, K=81, lddy=88, ldx=88, acc=1),
    _c(id="tail-83-83", M=200, N=81, K=81, lddy=83, ldx=83),
    _c(id="tail-88-88-ptr", M=200, N=81, K=81, lddy=88, ldx=88, dyo=1, xo=1),
    _c(id="tail-splits", M=600, N=81, K=81, lddy=88, ldx=96, acc=1),
    _c(id="xf32-ldx84", M=200, N=40, K=81, ldx=84, xf32=True, dts=H16),
    _c(id="xf32-splits", M=1000, N=40, K=81, ldx=81, xf32=True, acc=1, dts=H16),
]
LIN_WGRAD_RANDOM = [
    _c(id="one-split", M=200, N=40, K=81, lddy=48, ldx=88),
    _c(id="one-split-acc", M=200, N=40, K=81, acc=1),
    _c(id="splits-acc", M=1000, N=43, K=81, lddy=48, ldx=88, acc=1),
    _c(id="t128", M=4200, N=130, K=130),
    _c(id="chunks512", M=8200, N=8, K=5, acc=1),
    _c(id="xf32", M=1000, N=40, K=81, xf32=True, dts=H16),
]

# LayerNorm: z[M,E] ldz, y (forward) and dy (backward) [rows,E] ldy, dz ldz2.  offsets zo, yo, dzo.  mp = (B, T, off)
LN_SCALAR_E = [(1, 1), (33, 33), (64, 65), (65, 65), (129, 129), (257, 257), (513, 513), (1023, 1023)]   # (E, stride)
LN_VECTOR_E = [4, 8, 40, 96, 500, 1000, 1016, 1024]
LN_CASES = (
    [_c(id=f"scalar-E{E}", M=11, E=E, ldz=ld, ldy=ld, lddz=ld) for E, ld in LN_SCALAR_E]
    + [_c(id=f"vector-E{E}", M=(37 if E < 1000 else 9), E=E, ldz=E + 8, ldy=E + 16, lddz=E + 24) for E in LN_VECTOR_E]
    + [_c(id="fallback-ldz", M=11, E=64, ldz=65, ldy=72, lddz=72),
       _c(id="fallback-ldy", M=11, E=64, ldz=72, ldy=65, lddz=72),
       _c(id="fallback-ptr", M=11, E=64, ldz=72, ldy=72, lddz=72, zo=1),
       _c(id="fallback-lddz", M=11, E=64, ldz=72, ldy=72, lddz=65, fwd=False),
       _c(id="M1-vector", M=1, E=64, ldz=64, ldy=64, lddz=64),
       _c(id="M1-scalar", M=1, E=33, ldz=33, ldy=33, lddz=33),
       _c(id="grid-stride-vector", M=40001, E=128, ldz=128, ldy=128, lddz=128, bwd=False),
       _c(id="grid-stride-scalar", M=40001, E=33, ldz=33, ldy=33, lddz=33, bwd=False),
       _c(id="empty-blocks", M=1000, E=8, ldz=8, ldy=8, lddz=8),
       _c(id="offset-row-vector", M=9, E=96, ldz=96, ldy=96, lddz=96, special=True),
       _c(id="offset-row-scalar", M=9, E=33, ldz=33, ldy=33, lddz=33, special=True)]
    + [_c(id=f"acc{a}-{'g' if g else ''}{'b' if b else ''}-E{E}", M=300, E=E, ldz=E, ldy=E, lddz=E, acc=a, dgamma=g, dbeta=b,
          fwd=False) for a in (0, 1) for g, b in ((True, True), (True, False), (False, True)) for E in (40, 33)]
)
LN_MAPS = [_c(id=f"E{E}-B{B}-T{T}-off{off}-pos{int(p)}", M=B * T, E=E, ldz=E, ldy=E + (8 if E % 8 == 0 else 2), lddz=E,
              mp=(B, T, off), pos=p)
           for E in (40, 33) for B in (1, 3) for T in (1, 7) for off in (0, 1) for p in (False, True)]


def case_dts(c):
    return c.get("dts", ALL)


def lin_fwd_branches(c, dt):
    M, N, K = c["M"], c["N"], c["K"]
    xf32 = c.get("xf32", False)
    ex = 4 if (xf32 or dt == "f32") else 2
    others = []
    if c.get("ldr"):
        others.append((c["ldr"], c.get("ro", 0)))
    if c.get("pre"):
        others.append((c.get("ldy", N), c.get("po", 0)))
    return {"tile": fwd_tile(dt, xf32, M, N, K), "stage_x": stage_branch(ex, c.get("ldx", K), K, c.get("xo", 0)),
            "store": store_branch(dt, N, c.get("ldy", N), c.get("yo", 0), others), "k_tiles": "one" if K <= (32 if dt == "f32" else 64) else "many"}


def lin_dgrad_branches(c, dt):
    M, N, K = c["M"], c["N"], c["K"]
    others = []
    if c.get("act") and c.get("lds"):
        others.append((c["lds"], c.get("so", 0)))
    if c.get("lddr"):
        others.append((c["lddr"], c.get("ro", 0)))
    return {"tile": dgrad_tile(dt, M, N, K), "stage_dy": stage_branch(ESIZE[dt], c.get("lddy", N), N, c.get("dyo", 0)),
            "store": store_branch(dt, K, c.get("lddx", K), c.get("dxo", 0), others)}


def lin_wgrad_branches(c, dt):
    M, N, K = c["M"], c["N"], c["K"]
    xf32 = c.get("xf32", False)
    acc = c.get("acc", 0)
    out = {"stage_dy": stage_branch(ESIZE[dt], c.get("lddy", N), N, c.get("dyo", 0)),
           "stage_x": stage_branch(4 if (xf32 or dt == "f32") else 2, c.get("ldx", K), K, c.get("xo", 0))}
    if c.get("dW", True):
        out["tile"] = wgrad_tile(dt, xf32, M, N, K)
        out["dW"] = ("slabs" if wgrad_launch(M, N, K)[1] > 1 else "in-kernel") + ("-acc" if acc else "")
    if c.get("db", True):
        out["db"] = colsum_regime(M, acc)
    return out
