"""The five fused encoder-layer blocks (csrc/fused_fwd.hip, csrc/fused_bwd.hip) against fp64 references that round what the
kernels round, in bf16 and fp16, at both compiled widths (E = 128 / F = 256 / head dim 32 and E = 64 / F = 128 / head dim 16).

One reference per block, `rnd` = rounding to the element type (None: nothing rounded).  Read off the kernels:
  * mlp_block_fwd (fused_fwd.hip:304-415).  The input affine is folded while the weights are staged: `stage_folded` (:180-206)
    makes the operand image r(W1 * gin), `fold_bias` (:207-224) b1' = b1 + W1 . bin with the UNFOLDED element-type W1, in fp32.
    u = n_in @ r(W1 * gin)^T + b1' accumulates in fp32; h = act(u) in fp32; `pack8` (:397) rounds h for fc2; the residual
    z = gin * n_in + (b2 + bin) + r(h) @ W2^T stays fp32 (:362-364, :320).  The u / h extras are the rounded fp32 values (:392-395).
  * attn_block_fwd (:438-768).  q rows: r(Wq * gin * QSCALE), QSCALE = 1/sqrt(Dh) * log2(e) in fp32 (:38, :43, :452); k, v rows
    r(W * gin); the folded bias (b + W . bin), times QSCALE on the q rows (:454).  q, k, v accumulate in fp32 and are rounded as
    MFMA operands (`pack8`, :543-544, :575).  Scores are in the log2 domain; P = exp2(s - max) * rcp(sum) in fp32, rounded before
    P V (:685-701); ctx is rounded before the out-projection and stored as exactly that operand (:707-708).  z = gin * n_in +
    (bo + bin) + r(ctx) @ Wo^T in fp32 (:455, :731).  The qkv extra stores q from the fp32 accumulator divided by QSCALE (:548),
    k as the rounded operand, v from an fp32 accumulator.
  * LayerNorm epilogue of both (`ln_store`, :256-282): mean, variance and rstd = rsqrt(var + 1e-5) in fp32; n = (z - mu) * rstd,
    x = gout * n + bout from the UNROUNDED fp32 n; every output rounded once.
  * mlp_block_bwd (fused_bwd.hip:122-433 four waves, :448-741 eight).  Phase 0: dz2 = rstd2 * (g2 dy - mean(g2 dy) - n2 mean(g2
    dy n2)) in fp32, rounded into the image DZ (:246-247); x1 = r(gamma1 * n1 + beta1) into the image X (:251-252): the
    backward does NOT fold the affine.  Phase 1: u = X @ W1^T + b1 (:283-299), so forward and backward form u differently; h =
    act(u) and dh = (DZ @ W2) * act'(u) in fp32, both rounded (hB, dhB, and the DH image, :316-320); dW1 = r(dh)^T X, dW2 =
    DZ^T r(h) (:338-339); dx1 = r(dh) @ W1 + DZ (:379-398).  db1 sums the unrounded dh (:310), db2 the unrounded dz2, dgamma2 /
    dbeta2 dy * n2 and dy (:240-246).
  * attn_out_bwd (:769-908): dz1 as dz2 above, rounded for the MFMAs (DZ) and the output; dctx = DZ @ Wo, dWo = DZ^T ctx;
    dbo sums the unrounded dz1.
  * qkv_bwd (:946-1058): dx = dqkv @ W + res, dW = dqkv^T x, db = column sums, every operand already element-type; the affine
    fix-up (mivit_qkv_bwd_affine) turns dW into dW diag(gamma) + db (x) beta.

Errors are normalised per row: row-wise outputs (u, h, z, n, x, ctx, qkv, dx1, dz1, dctx, dx) per activation row, max |got - ref|
/ max |ref| over the row; reduced outputs (dW*, db*, dgamma*, dbeta*) per output row of the parameter, a vector being one row.
rstd and mean are checked element-wise (relative, mean against the row's scale).  Bars: row-wise bf16 1e-2 / fp16 2e-3,
reduced bf16 1e-3 / fp16 5e-4, rstd and mean 1e-4; attn_block_fwd's rstd and mean bf16 2.5e-3 / fp16 5e-4 and its bf16 ctx 1.5e-2 (the
mechanism and the measured numbers are at BAR_ATTN).  Since a wrong LayerNorm epsilon moves rstd by only ~4e-5 at unit
variance, test_layernorm_epsilon_small_variance runs rows of variance ~1e-3, where it is a 5 % effect.  The kernel forms a rounded intermediate in fp32, the reference in fp64: an element
whose value lies within the fp32 error of a rounding boundary may round the other way, and a ReLU / leaky unit whose u lies within
that error of 0 may take the other derivative.  The backward references mark such elements (`flips`, `ambiguous`) and the bar
is widened by what they can move -- three standard deviations of the random-signed one-ulp flips, the full value for a derivative
flip -- so that a single flipped element of a one-row problem does not fail a 5e-4 bar, and nothing else is allowed.

Coverage: every dtype x width x block at one workgroup and at >= 2 passes of the persistent grid with a ragged last tile; every
(row tiles, extras, waves) instantiation of attn_block_fwd; every activation instantiation of both MLP blocks and both waves of
mlp_block_bwd; both input-affine modes; qkv_bwd with and without the fix-up; both slab-reduction branches; exact small-integer
and exact folded-affine tests; placement (NaN-filled outputs, sentinel guard rows); fp16 gradients in the subnormal range.
The tests without the `gpu` mark check the references against autograd, the visibility of the rounding model and the dispatch
coverage on the CPU.
"""
import ctypes
import math
import zlib

import numpy as np
import pytest
import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BAR_ROW = {"bf16": 1e-2, "f16": 2e-3}
BAR_RED = {"bf16": 1e-3, "f16": 5e-4}
BAR_RSTD = 1e-4
# attn_block_fwd rounds q, k, v and P besides ctx; their flips are not followed through the softmax by the reference, and they
# move ctx by a few ulps and z, hence rstd, with it.  An fp32 emulation of the kernel's arithmetic with the same roundings gives
# 3.79e-4 on rstd at B = 3, S = 31 (bf16, width 128), the kernel 3.80e-4.  Over 136 k rows the worst rstd reaches 1.81e-3
# (bf16) and 3.05e-4 (fp16) -- in the ratio of the two element types' ulps --, the mean 2.61e-4 of its row's scale (bf16), and
# ctx 1.22e-2 of its row (bf16).  These bars apply to attn_block_fwd's rstd and mean.
BAR_ATTN = {"rstd": {"bf16": 2.5e-3, "f16": 5e-4}, "ctx_bf16": 1.5e-2}
QUARTER_ULP = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12}   # a quarter ulp, relative, at the top of a binade
PREC = {"bf16": 8, "f16": 11}                       # significant bits
WIDTHS = {128: (128, 256, 32), 64: (64, 128, 16)}   # E, F, head dim
H = 4
BENCH_M = 140017                                    # bench-scale rows: > 2 passes of every persistent grid, ragged last tile
ACT_NAMES = {0: "none", 1: "relu", 2: "leaky", 3: "gelu"}

_WORST = {}     # (block, dtype, width) -> (worst error / bar, error, what)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (blk, dt, w), (ratio, e, what) in sorted(_WORST.items()):
        print(f"[fused blocks] {blk:14s} {dt:4s} w{w:<3d} worst {e:.3e} = {ratio:.2f} of its bar  ({what})")


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def qscale(Dh):
    """fused_fwd.hip: constexpr float QSCALE = (1/sqrt(Dh)) * log2(e), a product of two fp32 constants"""
    inv = {32: 0.17677669529663687, 16: 0.25}[Dh]
    return float(np.float32(inv) * np.float32(1.4426950408889634))


def rounder(dt):
    if dt is None:
        return None
    t = DT[dt]

    def rnd(x):
        return x.to(t).to(x.dtype)
    rnd.dt = dt
    return rnd


def _r(rnd, x):
    return rnd(x) if rnd else x


def act_f(act, u):
    if act == 1:
        return torch.relu(u)
    if act == 2:
        return torch.where(u > 0, u, 0.01 * u)
    if act == 3:
        return 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))
    return u


def act_d(act, u):
    if act == 1:
        return (u > 0).to(u.dtype)
    if act == 2:
        return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, 0.01))
    if act == 3:
        return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    return torch.ones_like(u)


def ln_ref(z):
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + 1e-5)
    return (z - mu) * rstd, mu.squeeze(-1), rstd.squeeze(-1)


def ln_bwd(dy, n, rstd, g):
    gdy = dy * g
    return rstd[:, None] * (gdy - gdy.mean(-1, keepdim=True) - n * (gdy * n).mean(-1, keepdim=True))


def mlp_fwd_ref(n, gin, bin_, W1, b1, W2, b2, gout, bout, act, rnd=None):
    """all arguments float64 (n and the weights hold element-type values); gin / bin_ None = identity affine"""
    E = n.shape[-1]
    gi = gin if gin is not None else torch.ones(E, dtype=n.dtype, device=n.device)
    bi = bin_ if bin_ is not None else torch.zeros(E, dtype=n.dtype, device=n.device)
    W1i = _r(rnd, W1 * gi) if gin is not None else W1
    b1f = b1 + W1 @ bi
    u = n @ W1i.t() + b1f
    h = act_f(act, u)
    z = gi * n + (b2 + bi) + _r(rnd, h) @ W2.t()
    nh, mu, rstd = ln_ref(z)
    out = dict(u=u, h=h, z=z, n=nh, x=nh * gout + bout, rstd=rstd, mean=mu)
    if rnd is not None:             # r(h) elements that may round the other way move z, hence rstd
        tol_u = ACC_TOL * (n.abs() @ W1i.abs().t() + b1f.abs())
        out["_rstd_slack"] = rstd_slack(z, mu, _sq(flips(h, tol_u * act_d(act, u).abs() + EW_TOL * h.abs(), dt_of(rnd)), W2.t()))
    return out


def rstd_slack(z, mu, zs):
    """relative change of rstd that a change of at most zs per element of z can cause: |d var| / (2 var)"""
    var = ((z - mu[..., None]) ** 2).mean(-1)
    return ((z - mu[..., None]).abs() * zs).mean(-1) * 2 / (2 * var)


def dt_of(rnd):
    return rnd.dt


def attn_fwd_ref(n, gin, bin_, Wqkv, bqkv, Wo, bo, gout, bout, rnd=None):
    """n [B, S, E] float64; returns the block's outputs [B, S, *] and rstd / mean [B, S]"""
    B, S, E = n.shape
    Dh = E // H
    qs = qscale(Dh)
    gi = gin if gin is not None else torch.ones(E, dtype=n.dtype, device=n.device)
    bi = bin_ if bin_ is not None else torch.zeros(E, dtype=n.dtype, device=n.device)
    scale = torch.ones(3 * E, 1, dtype=n.dtype, device=n.device)
    scale[:E] = qs
    Wimg = _r(rnd, Wqkv * gi * scale)
    bf = (bqkv + Wqkv @ bi) * scale[:, 0]
    acc = n @ Wimg.t() + bf                                 # fp32 accumulators: q carries QSCALE
    q, k, v = (_r(rnd, t).view(B, S, H, Dh).transpose(1, 2) for t in acc.split(E, dim=-1))
    s = q @ k.transpose(-1, -2)                             # log2 domain
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    pr = _r(rnd, p)
    ctx32 = (pr @ v).transpose(1, 2).reshape(B, S, E)
    ctx = _r(rnd, ctx32)
    z = gi * n + (bo + bi) + ctx @ Wo.t()
    nh, mu, rstd = ln_ref(z)
    qkv = torch.cat([acc[..., :E] / qs, acc[..., E:]], dim=-1)
    out = dict(ctx=ctx, z=z, n=nh, x=nh * gout + bout, rstd=rstd, mean=mu, qkv=qkv)
    if rnd is not None:             # ctx elements that may round the other way move z, hence rstd
        tol = ACC_TOL * (pr.abs() @ v.abs()).transpose(1, 2).reshape(B, S, E)
        out["_rstd_slack"] = rstd_slack(z, mu, _sq(flips(ctx32, tol, dt_of(rnd)), Wo.t()))
    return out


def ulp(x, dt):
    """spacing of the element type at |x| (fp16 subnormals included)"""
    _, e = torch.frexp(x.abs())
    u = torch.ldexp(torch.ones_like(x), e - PREC[dt])
    return u.clamp_min(2.0 ** -24) if dt == "f16" else u


def flips(x, tol, dt):
    """one ulp where rounding x to the element type may differ between the kernel's fp32 value and the fp64 one (x within
    `tol` of a rounding boundary), 0 elsewhere"""
    if dt is None:
        return torch.zeros_like(x)
    u = ulp(x, dt)
    near = (u / 2 - (x - rounder(dt)(x)).abs()) <= tol
    return torch.where(near, u, torch.zeros_like(x))


F16_FLOOR = 2.0 ** -22         # fp16's absolute resolution is 2^-24: four subnormal ulps on a row-wise fp16 gradient
ACC_TOL = 2.0 ** -21           # fp32 error of an accumulation over <= 4 MFMA steps (one rounding each), relative to sum |terms|
EW_TOL = 2.0 ** -22            # ... of an element-wise expression


def _sq(a, b):
    """3 standard deviations of a sum of random-signed terms bounded by a_ij * b_jk"""
    return 3 * torch.sqrt((a * a) @ (b * b))


def mlp_bwd_ref(dy, n2, rstd2, g2, n1, g1, be1, W1, b1, W2, act, rnd=None, dt=None):
    """float64 arguments; returns (reference dict, slack dict): slack bounds what rounding flips and derivative flips at
    u ~ 0 (see the module docstring) can move each output element"""
    dz = ln_bwd(dy, n2, rstd2, g2)
    x1v = g1 * n1 + be1
    X = _r(rnd, x1v)
    u = X @ W1.t() + b1
    h = act_f(act, u)
    gr = _r(rnd, dz) @ W2
    dh = gr * act_d(act, u)
    DZ, hB, dhB = _r(rnd, dz), _r(rnd, h), _r(rnd, dh)
    ref = dict(dx1=dhB @ W1 + DZ, dW1=dhB.t() @ X, db1=dh.sum(0), dW2=DZ.t() @ hB, db2=dz.sum(0),
               dgamma2=(dy * n2).sum(0), dbeta2=dy.sum(0))
    slack = {k: torch.zeros_like(v) for k, v in ref.items()}
    if rnd is None:
        return ref, slack
    gdy = (dy * g2).abs()
    tol_dz = ACC_TOL * rstd2[:, None] * (gdy + gdy.mean(-1, keepdim=True) + n2.abs() * (gdy * n2.abs()).mean(-1, keepdim=True))
    fX = flips(x1v, EW_TOL * ((g1 * n1).abs() + be1.abs()), dt)
    fDZ = flips(dz, tol_dz, dt)
    # (a flipped element of X or DZ moves u or dh by far more than the fp32 error: it widens their uncertainty)
    tol_u = ACC_TOL * (X.abs() @ W1.abs().t() + b1.abs()) + fX @ W1.abs().t()
    tol_g = ACC_TOL * (DZ.abs() @ W2.abs()) + fDZ @ W2.abs()
    ad = act_d(act, u).abs()
    fh = flips(h, tol_u * ad + EW_TOL * h.abs(), dt)
    fdh = flips(dh, tol_g * ad + EW_TOL * dh.abs() + (gr.abs() * tol_u if act == 3 else 0), dt)
    if act in (1, 2):
        amb = (u.abs() <= tol_u).to(u.dtype) * gr.abs() * (0.99 if act == 2 else 1.0)
    else:
        amb = torch.zeros_like(u)
    slack["dx1"] = amb @ W1.abs() + _sq(fdh, W1) + fDZ + (F16_FLOOR if dt == "f16" else 0)
    slack["dW1"] = amb.t() @ X.abs() + _sq(fdh.t(), X) + _sq(dhB.abs().t(), fX)
    slack["db1"] = amb.sum(0)
    slack["dW2"] = _sq(fDZ.t(), hB) + _sq(DZ.abs().t(), fh)
    slack["_ambiguous"] = float((amb > 0).double().mean())
    slack["_flagged"] = max(float((f > 0).double().mean()) for f in (fX, fDZ, fh, fdh))
    return ref, slack


def attn_out_bwd_ref(dy, n1, rstd1, g1, ctx, Wo, rnd=None, dt=None):
    dz = ln_bwd(dy, n1, rstd1, g1)
    DZ = _r(rnd, dz)
    ref = dict(dz1=dz, dctx=DZ @ Wo, dWo=DZ.t() @ ctx, dbo=dz.sum(0), dgamma1=(dy * n1).sum(0), dbeta1=dy.sum(0))
    slack = {k: torch.zeros_like(v) for k, v in ref.items()}
    if rnd is not None:
        gdy = (dy * g1).abs()
        tol = ACC_TOL * rstd1[:, None] * (gdy + gdy.mean(-1, keepdim=True) + n1.abs() * (gdy * n1.abs()).mean(-1, keepdim=True))
        fDZ = flips(dz, tol, dt)
        slack["dctx"] = _sq(fDZ, Wo)
        slack["dWo"] = _sq(fDZ.t(), ctx)
    return ref, slack


def qkv_bwd_ref(dqkv, x, W, res, fix_gamma=None, fix_beta=None):
    dW, db = dqkv.t() @ x, dqkv.sum(0)
    if fix_gamma is not None:
        dW = dW * fix_gamma + db[:, None] * fix_beta
    ref = dict(dx=dqkv @ W + res, dW=dW, db=db)
    return ref, {k: torch.zeros_like(v) for k, v in ref.items()}


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
ROWWISE = {"u", "h", "z", "n", "x", "ctx", "qkv", "dx1", "dz1", "dctx", "dx"}


def row_err(got, ref, slack=None):
    """per row: max over the row of (|got - ref| - slack)+ / max |ref| (a row whose reference is zero must be zero)"""
    got, ref = got.double().reshape(-1, got.shape[-1]) if got.dim() > 1 else got.double()[None], \
        ref.double().reshape(-1, ref.shape[-1]) if ref.dim() > 1 else ref.double()[None]
    d = (got - ref).abs()
    if slack is not None:
        s = slack.double().reshape(d.shape)
        d = (d - s).clamp_min(0)
    d[torch.isnan(got)] = math.inf
    m = ref.abs().amax(-1)
    dm = d.amax(-1)
    return torch.where(m > 0, dm / m.clamp_min(1e-300), torch.where(dm > 0, torch.full_like(dm, math.inf), torch.zeros_like(dm)))


def check(block, dt, w, got, ref, slack=None, what="", keys=None):
    """every output in `ref` (or `keys`) within its bar; records the worst error per (block, dtype, width)"""
    slack = slack or {}
    for k in keys or ref:
        g, r = got[k], ref[k].to(got[k].device)
        if k == "rstd":
            e = ((g.double() - r) / r).abs()
            if "_rstd_slack" in ref:
                e = (e - ref["_rstd_slack"].to(e.device)).clamp_min(0)
            e = e.max()
            bar = BAR_ATTN["rstd"][dt] if block == "attn_block_fwd" else BAR_RSTD
        elif k == "mean":
            scale = got["_zscale"] if "_zscale" in got else r.abs().max().clamp_min(1e-30)
            e = ((g.double() - r).abs() / scale).max()
            bar = BAR_ATTN["rstd"][dt] if block == "attn_block_fwd" else BAR_RSTD
        else:
            bar = BAR_ROW[dt] if k in ROWWISE else BAR_RED[dt]
            if block == "attn_block_fwd" and k == "ctx" and dt == "bf16":
                bar = BAR_ATTN["ctx_bf16"]
            s = slack.get(k)
            e = row_err(g, r, None if s is None else s.to(g.device))
            e = e.max()
        e = float(e)
        key = (block, dt, w)
        if key not in _WORST or e / bar > _WORST[key][0]:
            _WORST[key] = (e / bar, e, f"{k} {what}")
        assert e <= bar, f"{block} {dt} w{w} {what}: {k} off by {e:.3e} > {bar:.0e}"


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def randn(shape, seed, scale=1.0, device="cpu"):
    return torch.randn(*shape, generator=_gen(seed, device), device=device, dtype=torch.float32) * scale


def mlp_fwd_inputs(M, w, dt, affine, seed, device="cpu"):
    E, F, _ = WIDTHS[w]
    t = DT[dt]
    p = dict(n=randn((M, E), seed, device=device).to(t),
             gin=(1 + 0.3 * randn((E,), seed + 1, device=device)) if affine else None,
             bin=(0.2 * randn((E,), seed + 2, device=device)) if affine else None,
             W1=randn((F, E), seed + 3, 1 / math.sqrt(E), device).to(t), b1=0.1 * randn((F,), seed + 4, device=device),
             W2=randn((E, F), seed + 5, 1 / math.sqrt(F), device).to(t), b2=0.1 * randn((E,), seed + 6, device=device),
             gout=1 + 0.3 * randn((E,), seed + 7, device=device), bout=0.2 * randn((E,), seed + 8, device=device))
    return p


def attn_fwd_inputs(B, S, w, dt, affine, seed, device="cpu"):
    E, _, _ = WIDTHS[w]
    t = DT[dt]
    return dict(n=randn((B, S, E), seed, device=device).to(t),
                gin=(1 + 0.3 * randn((E,), seed + 1, device=device)) if affine else None,
                bin=(0.2 * randn((E,), seed + 2, device=device)) if affine else None,
                Wqkv=randn((3 * E, E), seed + 3, 1.5 / math.sqrt(E), device).to(t), bqkv=0.1 * randn((3 * E,), seed + 4, device=device),
                Wo=randn((E, E), seed + 5, 1 / math.sqrt(E), device).to(t), bo=0.1 * randn((E,), seed + 6, device=device),
                gout=1 + 0.3 * randn((E,), seed + 7, device=device), bout=0.2 * randn((E,), seed + 8, device=device))


def ln_inputs(M, E, dt, seed, device="cpu", dy_scale=1.0):
    """a consistent (normalised rows, rstd) pair: n = LNhat(z) rounded, rstd of z"""
    t = DT[dt]
    z = randn((M, E), seed, device=device) * (1 + randn((M, 1), seed + 1, device=device).abs())
    nh, _, rstd = ln_ref(z.double())
    return nh.to(t), rstd.float(), (randn((M, E), seed + 2, dy_scale, device)).to(t)


def mlp_bwd_inputs(M, w, dt, seed, device="cpu", dy_scale=1.0):
    E, F, _ = WIDTHS[w]
    t = DT[dt]
    n2, rstd2, dy = ln_inputs(M, E, dt, seed, device, dy_scale)
    return dict(dy=dy, n2=n2, rstd2=rstd2, gamma2=1 + 0.3 * randn((E,), seed + 3, device=device),
                n1=randn((M, E), seed + 4, device=device).to(t), gamma1=1 + 0.3 * randn((E,), seed + 5, device=device),
                beta1=0.2 * randn((E,), seed + 6, device=device),
                W1=randn((F, E), seed + 7, 1 / math.sqrt(E), device).to(t), b1=0.1 * randn((F,), seed + 8, device=device),
                W2=randn((E, F), seed + 9, 1 / math.sqrt(F), device).to(t))


def attn_out_bwd_inputs(M, w, dt, seed, device="cpu"):
    E, _, _ = WIDTHS[w]
    t = DT[dt]
    n1, rstd1, dy = ln_inputs(M, E, dt, seed, device)
    return dict(dy=dy, n1=n1, rstd1=rstd1, gamma1=1 + 0.3 * randn((E,), seed + 3, device=device),
                ctx=randn((M, E), seed + 4, device=device).to(t), Wo=randn((E, E), seed + 5, 1 / math.sqrt(E), device).to(t))


def qkv_bwd_inputs(M, w, dt, fix, seed, device="cpu"):
    E, _, _ = WIDTHS[w]
    t = DT[dt]
    return dict(dqkv=randn((M, 3 * E), seed, device=device).to(t), x=randn((M, E), seed + 1, device=device).to(t),
                Wqkv=randn((3 * E, E), seed + 2, 1 / math.sqrt(E), device).to(t), res=randn((M, E), seed + 3, device=device).to(t),
                fix_gamma=(1 + 0.3 * randn((E,), seed + 4, device=device)) if fix else None,
                fix_beta=(0.2 * randn((E,), seed + 5, device=device)) if fix else None)


def d64(p, device=None):
    return {k: (None if v is None else v.to(device or v.device).double()) for k, v in p.items()}


def ref_device(M):
    """fp64 references of small problems on the CPU; bench-scale ones in torch fp64 on the GPU (rocBLAS dgemm: a code path
    independent of the kernels under test)"""
    return "cuda" if M > 4096 else "cpu"


# ---------------------------------------------------------------------------------------------------------------------
# dispatch rules, restated
# ---------------------------------------------------------------------------------------------------------------------
def attn_instantiation(S, E, extras):
    """fused_fwd.hip::launch_attn_block_fwd -> (NT, EXTRAS, NW) of the kernel it launches"""
    nt = (S + 15) // 16
    nw = 4 if E == 128 and (nt >= 3 or extras) else 8
    return min(nt, 4), extras, nw


def attn_reachable(E):
    return {attn_instantiation(S, E, ex) for S in range(1, 65) for ex in (False, True)}


ATTN_S = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]


def test_dispatch_coverage():
    """the S list of test_attn_block_fwd reaches every (NT, EXTRAS, NW) instantiation the launcher can select, per width"""
    for E in (128, 64):
        hit = {attn_instantiation(S, E, ex) for S in ATTN_S for ex in (False, True)}
        assert hit == attn_reachable(E), (E, attn_reachable(E) - hit)
    assert len(attn_reachable(128)) == 8 and len(attn_reachable(64)) == 8       # 4 row-tile counts x lean / extras


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the references are the plain formulas, and the rounding model is visible at the bars
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_mlp_fwd_reference_is_the_formula(act):
    p = d64(mlp_fwd_inputs(9, 64, "bf16", True, _seed("mf", act)))
    r = mlp_fwd_ref(p["n"], p["gin"], p["bin"], p["W1"], p["b1"], p["W2"], p["b2"], p["gout"], p["bout"], act)
    x = p["gin"] * p["n"] + p["bin"]
    u = x @ p["W1"].t() + p["b1"]
    z = x + act_f(act, u) @ p["W2"].t() + p["b2"]
    nh = torch.nn.functional.layer_norm(z, (z.shape[-1],), eps=1e-5)
    for k, v in (("u", u), ("z", z), ("n", nh), ("x", nh * p["gout"] + p["bout"])):
        torch.testing.assert_close(r[k], v, rtol=1e-12, atol=1e-12)


def test_attn_fwd_reference_is_the_formula():
    for w in (128, 64):
        E, _, Dh = WIDTHS[w]
        p = d64(attn_fwd_inputs(2, 19, w, "bf16", True, _seed("af", w)))
        r = attn_fwd_ref(p["n"], p["gin"], p["bin"], p["Wqkv"], p["bqkv"], p["Wo"], p["bo"], p["gout"], p["bout"])
        x = p["gin"] * p["n"] + p["bin"]
        mha = torch.nn.MultiheadAttention(E, H, batch_first=True, dtype=torch.float64)
        with torch.no_grad():
            mha.in_proj_weight.copy_(p["Wqkv"]); mha.in_proj_bias.copy_(p["bqkv"])
            mha.out_proj.weight.copy_(p["Wo"]); mha.out_proj.bias.copy_(p["bo"])
            a, _ = mha(x, x, x, need_weights=False)
        z = x + a
        nh = torch.nn.functional.layer_norm(z, (E,), eps=1e-5)
        # (QSCALE is an fp32 constant: the scores carry its rounding, 1e-8 relative)
        torch.testing.assert_close(r["z"], z, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(r["n"], nh, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(r["qkv"], x @ p["Wqkv"].t() + p["bqkv"], rtol=1e-12, atol=1e-12)


def _mlp_chain(p, act):
    """autograd of x2 = gamma2 * LN(x1 + fc2(act(fc1 x1))) + beta2, x1 = gamma1 * n1 + beta1, in fp64"""
    E = p["n1"].shape[-1]
    x1 = (p["gamma1"] * p["n1"] + p["beta1"]).requires_grad_()
    W1, b1, W2 = (p[k].clone().requires_grad_() for k in ("W1", "b1", "W2"))
    b2 = torch.zeros(E, dtype=torch.float64, requires_grad=True)
    g2, be2 = p["gamma2"].clone().requires_grad_(), torch.zeros(E, dtype=torch.float64, requires_grad=True)
    z = x1 + act_f(act, x1 @ W1.t() + b1) @ W2.t() + b2
    nh, _, rstd = ln_ref(z)
    dy = torch.randn(nh.shape, generator=_gen(7), dtype=torch.float64)
    ((g2 * nh + be2) * dy).sum().backward()
    return nh.detach(), rstd.detach(), dy, dict(dx1=x1.grad, dW1=W1.grad, db1=b1.grad, dW2=W2.grad, db2=b2.grad, dgamma2=g2.grad,
                                               dbeta2=be2.grad)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_mlp_bwd_reference_is_autograd(act):
    p = d64(mlp_bwd_inputs(13, 64, "bf16", _seed("mb", act)))
    nh, rstd, dy, auto = _mlp_chain(p, act)
    r, s = mlp_bwd_ref(dy, nh, rstd, p["gamma2"], p["n1"], p["gamma1"], p["beta1"], p["W1"], p["b1"], p["W2"], act)
    for k, v in auto.items():
        torch.testing.assert_close(r[k], v, rtol=1e-10, atol=1e-10)
        assert float(s[k].abs().max()) == 0


def test_attn_out_and_qkv_bwd_references_are_autograd():
    M, E = 11, 64
    g = _gen(3)
    xin = torch.randn(M, E, generator=g, dtype=torch.float64)
    ctx = torch.randn(M, E, generator=g, dtype=torch.float64)
    Wo = torch.randn(E, E, generator=g, dtype=torch.float64).requires_grad_()
    bo = torch.zeros(E, dtype=torch.float64, requires_grad=True)
    ctx_ = ctx.clone().requires_grad_()
    g1, be1 = (1 + 0.3 * torch.randn(E, generator=g, dtype=torch.float64)).requires_grad_(), torch.zeros(E, dtype=torch.float64, requires_grad=True)
    zr = (xin + ctx_ @ Wo.t() + bo).requires_grad_()
    zr.retain_grad()
    nh, _, rstd = ln_ref(zr)
    dy = torch.randn(M, E, generator=g, dtype=torch.float64)
    ((g1 * nh + be1) * dy).sum().backward()
    r, _ = attn_out_bwd_ref(dy, nh.detach(), rstd.detach(), g1.detach(), ctx, Wo.detach())
    for k, v in dict(dz1=zr.grad, dctx=ctx_.grad, dWo=Wo.grad, dbo=bo.grad, dgamma1=g1.grad, dbeta1=be1.grad).items():
        torch.testing.assert_close(r[k], v, rtol=1e-10, atol=1e-10)
    n = torch.randn(M, E, generator=g, dtype=torch.float64)
    fg, fb = 1 + 0.3 * torch.randn(E, generator=g, dtype=torch.float64), torch.randn(E, generator=g, dtype=torch.float64)
    W = torch.randn(3 * E, E, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.zeros(3 * E, dtype=torch.float64, requires_grad=True)
    xt = (fg * n + fb).requires_grad_()
    dqkv, res = torch.randn(M, 3 * E, generator=g, dtype=torch.float64), torch.randn(M, E, generator=g, dtype=torch.float64)
    ((xt @ W.t() + b) * dqkv).sum().add((xt * res).sum()).backward()
    r, _ = qkv_bwd_ref(dqkv, n, W.detach(), res, fg, fb)
    for k, v in dict(dx=xt.grad, dW=W.grad, db=b.grad).items():
        torch.testing.assert_close(r[k], v, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rounding_model_is_visible_at_the_bars(dt):
    """With rounding on, the references move by about an ulp of the element type from the unrounded ones: row-wise outputs by
    less than a few ulps of their row, and at M = 1 a reduced gradient by more than a quarter ulp.  For bf16 that is more than
    its 1e-3 bar, so a reference with the wrong rounding model fails it; for fp16 (quarter ulp 2.4e-4, measured 4.7e-4 on dWo
    against the 5e-4 bar) the bar sits just above the rounding model's own effect."""
    rnd, two_ulp = rounder(dt), 2.0 ** (2 - PREC[dt])
    p = d64(mlp_fwd_inputs(31, 128, dt, True, _seed("vis", dt)))
    args = [p[k] for k in ("n", "gin", "bin", "W1", "b1", "W2", "b2", "gout", "bout")]
    a, b = mlp_fwd_ref(*args, 1, rnd), mlp_fwd_ref(*args, 1)
    for k in ("u", "z", "n"):
        e = float(row_err(a[k], b[k]).max())
        assert 0 < e < two_ulp, (k, e)
    pa = d64(attn_fwd_inputs(2, 33, 128, dt, True, _seed("vis-a", dt)))
    argsa = [pa[k] for k in ("n", "gin", "bin", "Wqkv", "bqkv", "Wo", "bo", "gout", "bout")]
    a, b = attn_fwd_ref(*argsa, rnd), attn_fwd_ref(*argsa)
    for k in ("ctx", "z", "n"):
        e = float(row_err(a[k], b[k]).max())
        assert 0 < e < 4 * two_ulp, (k, e)
    q = d64(mlp_bwd_inputs(1, 128, dt, _seed("vis-b", dt)))
    argsb = [q[k] for k in ("dy", "n2", "rstd2", "gamma2", "n1", "gamma1", "beta1", "W1", "b1", "W2")]
    (a, _), (b, _) = mlp_bwd_ref(*argsb, 3, rnd, dt), mlp_bwd_ref(*argsb, 3)
    assert float(row_err(a["dx1"], b["dx1"]).max()) < 4 * two_ulp
    assert max(float(row_err(a[k], b[k]).max()) for k in ("dW1", "dW2")) > QUARTER_ULP[dt]
    o = d64(attn_out_bwd_inputs(1, 128, dt, _seed("vis-o", dt)))
    (a, _), (b, _) = (attn_out_bwd_ref(*[o[k] for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")], rnd, dt),
                      attn_out_bwd_ref(*[o[k] for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")]))
    assert float(row_err(a["dWo"], b["dWo"]).max()) > QUARTER_ULP[dt]


def test_flip_slack_is_rare():
    """the allowance for rounding flips and derivative flips stays within the bars it widens (it must not turn into a blanket
    tolerance): measured at M = 4000, ReLU, width 128 -- about 1e-5 of the units ambiguous, 1 % (bf16) / 8 % (fp16) of the
    rounded elements flagged, and a median allowance on dW1 / dW2 rows of 0.9 (bf16) / 0.6 (fp16) of the reduced bar"""
    for dt in ("bf16", "f16"):
        q = d64(mlp_bwd_inputs(4000, 128, dt, _seed("slack", dt)))
        args = [q[k] for k in ("dy", "n2", "rstd2", "gamma2", "n1", "gamma1", "beta1", "W1", "b1", "W2")]
        ref, slack = mlp_bwd_ref(*args, 1, rounder(dt), dt)
        assert slack["_ambiguous"] < 1e-4, (dt, slack["_ambiguous"])
        assert slack["_flagged"] < 0.1, (dt, slack["_flagged"])
        for k in ("dW1", "dW2"):
            med = float((slack[k].amax(-1) / ref[k].abs().amax(-1)).median())
            assert med < BAR_RED[dt], (dt, k, med)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: raw C-ABI access (placement, slab branches)
# ---------------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _entry(name, w, dt):
    from moleculardiffusion_mivit_amd import _native as N
    return getattr(N.lib, name + ("_w64" if w == 64 else "") + ("_f16" if dt == "f16" else ""))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, w, dt, *args):
    from moleculardiffusion_mivit_amd import _native as N
    N.check(_entry(name, w, dt)(*args), name)


def _cuda(p):
    return {k: (None if v is None else v.cuda()) for k, v in p.items()}


GUARD = 37          # guard rows behind every row-wise output
SENTINEL = 1234.5   # exactly representable in bf16 and fp16


def _guarded(rows, cols, dtype):
    """(buffer with GUARD sentinel rows behind `rows` NaN rows, view of the in-range part)"""
    shape = (rows + GUARD, cols) if cols else (rows + GUARD,)
    buf = torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    buf[:rows] = float("nan")
    return buf, buf[:rows]


def _check_guarded(name, buf, rows):
    inr, guard = buf[:rows], buf[rows:]
    assert bool(torch.isfinite(inr).all()), f"{name}: {int((~torch.isfinite(inr)).sum())} in-range elements never written"
    assert bool((guard == SENTINEL).all()), f"{name}: guard rows overwritten"


# ---------------------------------------------------------------------------------------------------------------------
# GPU: mlp_block_fwd
# ---------------------------------------------------------------------------------------------------------------------
def _mlp_fwd_run(p, act, extras):
    from moleculardiffusion_mivit_amd import ops
    return ops.mlp_block_fwd(p["n"], p["gin"], p["bin"], p["W1"], p["b1"], p["W2"], p["b2"], p["gout"], p["bout"], act=act,
                             extras=extras)


def _mlp_fwd_case(w, dt, M, act, affine, extras=True):
    p = mlp_fwd_inputs(M, w, dt, affine, _seed("mlpf", w, dt, M, act, affine))
    dev = ref_device(M)
    q = d64(p, dev)
    ref = mlp_fwd_ref(q["n"], q["gin"], q["bin"], q["W1"], q["b1"], q["W2"], q["b2"], q["gout"], q["bout"], act, rounder(dt))
    out = _mlp_fwd_run(_cuda(p), act, extras)
    torch.cuda.synchronize()
    got = {k: v.to(dev) for k, v in out.items()}
    got["_zscale"] = ref["z"].abs().amax(-1)
    keys = ["n", "x", "z", "rstd", "mean", "u", "h"] if extras else ["n", "rstd"]
    check("mlp_block_fwd", dt, w, got, ref, what=f"M={M} act={ACT_NAMES[act]} affine={affine} extras={extras}", keys=keys)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 31, 33])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("affine", [False, True])
def test_mlp_block_fwd(w, dt, M, act, affine):
    out = _mlp_fwd_case(w, dt, M, act, affine)
    lean = _mlp_fwd_case(w, dt, M, act, affine, extras=False)
    assert torch.equal(lean["n"], out["n"]) and torch.equal(lean["rstd"], out["rstd"])


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_layernorm_epsilon_small_variance(w, dt):
    """Rows of variance ~1e-3: rstd depends on the LayerNorm epsilon at the 5 % level there (at unit variance a wrong epsilon
    of 1e-4 moves rstd by 4e-5 only, under the rstd bar), for both forward blocks."""
    from moleculardiffusion_mivit_amd import ops
    E = WIDTHS[w][0]
    p = mlp_fwd_inputs(33, w, dt, True, _seed("eps-m", w, dt))
    for k in ("n", "W2"):
        p[k] = (p[k].float() * 0.03).to(DT[dt])
    for k in ("bin", "b1", "b2"):
        p[k] = p[k] * 0.03
    q = d64(p)
    ref = mlp_fwd_ref(q["n"], q["gin"], q["bin"], q["W1"], q["b1"], q["W2"], q["b2"], q["gout"], q["bout"], 1, rounder(dt))
    assert float(((ref["z"] - ref["mean"][:, None]) ** 2).mean(-1).max()) < 3e-3
    out = _mlp_fwd_run(_cuda(p), 1, False)
    torch.cuda.synchronize()
    check("mlp_block_fwd", dt, w, {k: v.cpu() for k, v in out.items()}, ref, what="small variance", keys=["n", "rstd"])
    a = attn_fwd_inputs(3, 33, w, dt, True, _seed("eps-a", w, dt))
    for k in ("n", "Wo"):
        a[k] = (a[k].float() * 0.03).to(DT[dt])
    for k in ("bin", "bqkv", "bo"):
        a[k] = a[k] * 0.03
    q = d64(a)
    ref = attn_fwd_ref(q["n"], q["gin"], q["bin"], q["Wqkv"], q["bqkv"], q["Wo"], q["bo"], q["gout"], q["bout"], rounder(dt))
    c = _cuda(a)
    out = ops.attn_block_fwd(c["n"], c["gin"], c["bin"], c["Wqkv"], c["bqkv"], c["Wo"], c["bo"], c["gout"], c["bout"])
    torch.cuda.synchronize()
    check("attn_block_fwd", dt, w, {k: v.cpu() for k, v in out.items()}, ref, what="small variance", keys=["n", "rstd"])


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_mlp_block_fwd_bench_scale(w, dt):
    _mlp_fwd_case(w, dt, BENCH_M, 2, True)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: attn_block_fwd
# ---------------------------------------------------------------------------------------------------------------------
def _attn_case(w, dt, B, S, affine, extras):
    from moleculardiffusion_mivit_amd import ops
    p = attn_fwd_inputs(B, S, w, dt, affine, _seed("attf", w, dt, B, S, affine))
    dev = ref_device(B * S)
    q = d64(p, dev)
    ref = attn_fwd_ref(q["n"], q["gin"], q["bin"], q["Wqkv"], q["bqkv"], q["Wo"], q["bo"], q["gout"], q["bout"], rounder(dt))
    c = _cuda(p)
    out = ops.attn_block_fwd(c["n"], c["gin"], c["bin"], c["Wqkv"], c["bqkv"], c["Wo"], c["bo"], c["gout"], c["bout"], extras=extras)
    torch.cuda.synchronize()
    got = {k: v.to(dev) for k, v in out.items()}
    got["_zscale"] = ref["z"].abs().amax(-1)
    keys = ["ctx", "n", "rstd"] + (["x", "z", "mean", "qkv"] if extras else [])
    check("attn_block_fwd", dt, w, got, ref, what=f"B={B} S={S} affine={affine} extras={extras}", keys=keys)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("S", ATTN_S)
@pytest.mark.parametrize("extras", [False, True])
def test_attn_block_fwd(w, dt, S, extras):
    _attn_case(w, dt, 3, S, True, extras)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("extras", [False, True])
def test_attn_block_fwd_identity_input_affine(w, dt, extras):
    _attn_case(w, dt, 5, 33, False, extras)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("S,extras", [(17, False), (33, True)])
def test_attn_block_fwd_bench_scale(w, dt, S, extras):
    """4133 sequences: > 2 passes of the persistent grid at 8 waves (2048 per pass) and 4 waves, ragged last pass"""
    _attn_case(w, dt, 4133, S, True, extras)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_attn_block_fwd_rejects_65_tokens(dt):
    from moleculardiffusion_mivit_amd import ops, _native as N
    c = _cuda(attn_fwd_inputs(1, 65, 128, dt, False, 1))
    with pytest.raises(N.MivitError, match="tokens per sequence"):
        ops.attn_block_fwd(c["n"], None, None, c["Wqkv"], c["bqkv"], c["Wo"], c["bo"], c["gout"], c["bout"])
    assert not ops.fused_layer_supported(128, 256, 4, 65, DT[dt]) and ops.fused_layer_supported(128, 256, 4, 64, DT[dt])


@pytest.mark.gpu
def test_fused_ops_refuse_other_dtypes():
    from moleculardiffusion_mivit_amd import ops
    c = _cuda(qkv_bwd_inputs(4, 128, "bf16", False, 1))
    with pytest.raises(TypeError):
        ops.qkv_bwd(c["dqkv"].float(), c["x"].float(), c["Wqkv"].float(), c["res"].float())
    with pytest.raises(TypeError):
        ops.qkv_bwd(c["dqkv"], c["x"].half(), c["Wqkv"], c["res"])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: mlp_block_bwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def waves(request):
    """mlp_block_bwd's kernel switch of the element type under test (width 128; width 64 has the four-wave kernel only)"""
    nw, dt = request.param          # (waves, element type)
    from moleculardiffusion_mivit_amd import _native as N
    fn = N.lib.mivit_mlp_block_bwd_set_waves_f16 if dt == "f16" else N.lib.mivit_mlp_block_bwd_set_waves
    old = fn(nw)
    yield nw
    fn(old)


def _mlp_bwd_case(w, dt, M, act, nw, dy_scale=1.0, seed_key="mlpb"):
    from moleculardiffusion_mivit_amd import ops
    p = mlp_bwd_inputs(M, w, dt, _seed(seed_key, w, dt, M, act), dy_scale=dy_scale)
    dev = ref_device(M)
    q = d64(p, dev)
    ref, slack = mlp_bwd_ref(*[q[k] for k in ("dy", "n2", "rstd2", "gamma2", "n1", "gamma1", "beta1", "W1", "b1", "W2")], act,
                             rounder(dt), dt)
    c = _cuda(p)
    out = ops.mlp_block_bwd(*[c[k] for k in ("dy", "n2", "rstd2", "gamma2", "n1", "gamma1", "beta1", "W1", "b1", "W2")], act=act)
    torch.cuda.synchronize()
    check("mlp_block_bwd", dt, w, {k: v.to(dev) for k, v in out.items()}, ref, slack,
          what=f"M={M} act={ACT_NAMES[act]} waves={nw}" + (f" dy~{dy_scale:g}" if dy_scale != 1 else ""))
    return p, out


MLP_BWD_VARIANTS = [(w, dt, (nw, dt)) for w, dt, nw in
                    [(128, "bf16", 8), (128, "bf16", 4), (128, "f16", 8), (128, "f16", 4), (64, "bf16", 4), (64, "f16", 4)]]


@pytest.mark.gpu
@pytest.mark.parametrize("w,dt,waves", MLP_BWD_VARIANTS, indirect=["waves"],
                         ids=[f"w{w}-{dt}-{nw[0]}waves" for w, dt, nw in MLP_BWD_VARIANTS])
@pytest.mark.parametrize("M", [1, 31, 33])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_mlp_block_bwd(w, dt, waves, M, act):
    _mlp_bwd_case(w, dt, M, act, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("w,dt,waves", MLP_BWD_VARIANTS, indirect=["waves"],
                         ids=[f"w{w}-{dt}-{nw[0]}waves" for w, dt, nw in MLP_BWD_VARIANTS])
def test_mlp_block_bwd_bench_scale(w, dt, waves):
    _mlp_bwd_case(w, dt, BENCH_M, 1, waves)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
def test_mlp_block_bwd_fp16_subnormal_gradients(w):
    """dy ~ 1e-5: dz2, dh and dx1 fall into fp16's subnormal range (< 6.1e-5); the fp16 conversions and MFMAs must keep them"""
    p, out = _mlp_bwd_case(w, "f16", 1000, 3, 8 if w == 128 else 4, dy_scale=1e-5, seed_key="subn")
    dx1 = out["dx1"].float().abs()
    assert float(((dx1 > 0) & (dx1 < 2.0 ** -14)).float().mean()) > 0.1          # the case does reach subnormals


# ---------------------------------------------------------------------------------------------------------------------
# GPU: attn_out_bwd, qkv_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _attn_out_case(w, dt, M):
    from moleculardiffusion_mivit_amd import ops
    p = attn_out_bwd_inputs(M, w, dt, _seed("aob", w, dt, M))
    dev = ref_device(M)
    q = d64(p, dev)
    ref, slack = attn_out_bwd_ref(*[q[k] for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")], rounder(dt), dt)
    c = _cuda(p)
    out = ops.attn_out_bwd(*[c[k] for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")])
    torch.cuda.synchronize()
    check("attn_out_bwd", dt, w, {k: v.to(dev) for k, v in out.items()}, ref, slack, what=f"M={M}")
    return p, out


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 31, 33, BENCH_M])
def test_attn_out_bwd(w, dt, M):
    _attn_out_case(w, dt, M)


def _qkv_case(w, dt, M, fix):
    from moleculardiffusion_mivit_amd import ops
    p = qkv_bwd_inputs(M, w, dt, fix, _seed("qkvb", w, dt, M, fix))
    dev = ref_device(M)
    q = d64(p, dev)
    ref, slack = qkv_bwd_ref(q["dqkv"], q["x"], q["Wqkv"], q["res"], q["fix_gamma"], q["fix_beta"])
    c = _cuda(p)
    out = ops.qkv_bwd(c["dqkv"], c["x"], c["Wqkv"], c["res"], fix_gamma=c["fix_gamma"], fix_beta=c["fix_beta"])
    torch.cuda.synchronize()
    check("qkv_bwd", dt, w, {k: v.to(dev) for k, v in out.items()}, ref, slack, what=f"M={M} fix={fix}")
    return p, out


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 31, 33, BENCH_M])
@pytest.mark.parametrize("fix", [False, True])
def test_qkv_bwd(w, dt, M, fix):
    _qkv_case(w, dt, M, fix)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the one-launch slab reduction (gradient outputs contiguous in the parameter arena's order), raw C-ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_slab_reduction_in_arena_order(w, dt):
    E, F, _ = WIDTHS[w]
    M = 20001
    # mlp_block_bwd: fc1.weight, fc1.bias, fc2.weight, fc2.bias, norm2.weight, norm2.bias
    p = _cuda(mlp_bwd_inputs(M, w, dt, _seed("slab-m", w, dt)))
    from moleculardiffusion_mivit_amd import ops
    sep = ops.mlp_block_bwd(*[p[k] for k in ("dy", "n2", "rstd2", "gamma2", "n1", "gamma1", "beta1", "W1", "b1", "W2")], act=3)
    sizes = [("dW1", F * E), ("db1", F), ("dW2", E * F), ("db2", E), ("dgamma2", E), ("dbeta2", E)]
    arena = torch.full((sum(n for _, n in sizes),), float("nan"), device="cuda")
    views, o = {}, 0
    for k, n in sizes:
        views[k] = arena[o:o + n]
        o += n
    nb = _entry("mivit_mlp_block_bwd_workspace_bytes", w, dt)(M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dx1 = torch.empty(M, E, dtype=DT[dt], device="cuda")
    _call("mivit_mlp_block_bwd", w, dt, *[_p(p[k]) for k in ("dy", "n2", "rstd2", "gamma2", "n1", "gamma1", "beta1", "W1", "b1", "W2")],
          M, 3, _p(dx1), *[_p(views[k]) for k, _ in sizes], _p(ws), nb, _stream())
    torch.cuda.synchronize()
    for k, _ in sizes:
        assert torch.equal(views[k], sep[k].reshape(-1)), k
    # attn_out_bwd: out_proj.weight, out_proj.bias, norm1.weight, norm1.bias
    a = _cuda(attn_out_bwd_inputs(M, w, dt, _seed("slab-a", w, dt)))
    sep = ops.attn_out_bwd(*[a[k] for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")])
    sizes = [("dWo", E * E), ("dbo", E), ("dgamma1", E), ("dbeta1", E)]
    arena = torch.full((sum(n for _, n in sizes),), float("nan"), device="cuda")
    views, o = {}, 0
    for k, n in sizes:
        views[k] = arena[o:o + n]
        o += n
    nb = _entry("mivit_attn_out_bwd_workspace_bytes", w, dt)(M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dz1, dctx = torch.empty(M, E, dtype=DT[dt], device="cuda"), torch.empty(M, E, dtype=DT[dt], device="cuda")
    _call("mivit_attn_out_bwd", w, dt, *[_p(a[k]) for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")], M, _p(dz1), _p(dctx),
          *[_p(views[k]) for k, _ in sizes], _p(ws), nb, _stream())
    torch.cuda.synchronize()
    for k, _ in sizes:
        assert torch.equal(views[k], sep[k].reshape(-1)), k
    # qkv_bwd (with the affine fix-up, as the engine runs it): in_proj weight, in_proj bias
    qv = _cuda(qkv_bwd_inputs(M, w, dt, True, _seed("slab-q", w, dt)))
    sep = ops.qkv_bwd(qv["dqkv"], qv["x"], qv["Wqkv"], qv["res"], fix_gamma=qv["fix_gamma"], fix_beta=qv["fix_beta"])
    arena = torch.full((3 * E * E + 3 * E,), float("nan"), device="cuda")
    nb = _entry("mivit_qkv_bwd_workspace_bytes", w, dt)(M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dx = torch.empty(M, E, dtype=DT[dt], device="cuda")
    _call("mivit_qkv_bwd_affine", w, dt, *[_p(qv[k]) for k in ("dqkv", "x", "Wqkv", "res")], M, _p(dx), _p(arena[:3 * E * E]),
          _p(arena[3 * E * E:]), _p(qv["fix_gamma"]), _p(qv["fix_beta"]), _p(ws), nb, _stream())
    torch.cuda.synchronize()
    assert torch.equal(arena[:3 * E * E], sep["dW"].reshape(-1)) and torch.equal(arena[3 * E * E:], sep["db"])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: exact tests (small integers; folded affine with gamma in {0.5, 1, 2} and small-integer beta)
# ---------------------------------------------------------------------------------------------------------------------
def _ints(shape, mod, off, mul, add):
    return ((torch.arange(int(np.prod(shape))).reshape(shape) * mul + add) % mod - off).float()


def _sparse(shape, mod, mul, add, vals):
    a = torch.arange(int(np.prod(shape))).reshape(shape)
    return (((a * mul + add) % mod) == 0).float() * ((a % vals) - (vals // 2))


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("affine", [False, True])
def test_mlp_block_fwd_exact(w, dt, affine):
    """Small integers (and, with the input affine, gamma in {0.5, 1, 2} and small-integer beta): W1 * gamma and b1 + W1 beta
    are exact, so every product and sum is exact; a gamma or beta applied to the wrong column, a missing bias chunk or a wrong
    permutation of the hidden index is an exact mismatch in u, h and z."""
    from moleculardiffusion_mivit_amd import ops
    E, F, _ = WIDTHS[w]
    M = 300
    n = _ints((M, E), 5, 2, 7, 3)
    W1 = _sparse((F, E), 23, 11, 1, 3)
    W2 = _sparse((E, F), 29, 5, 2, 5)
    b1, b2 = _ints((F,), 7, 3, 1, 0), _ints((E,), 5, 2, 1, 0)
    if affine:
        gin = torch.tensor([0.5, 1.0, 2.0])[(torch.arange(E) * 7 + 1) % 3]
        bin_ = _ints((E,), 5, 2, 3, 1)
    else:
        gin, bin_ = torch.ones(E), torch.zeros(E)
    x = gin * n + bin_
    u = x @ W1.t() + b1
    h = torch.relu(u)
    z = x + h @ W2.t() + b2
    assert float(z.abs().max()) <= 256 and float(u.abs().max()) <= 256       # exact in bf16 (8 bits) and fp16
    t = DT[dt]
    out = ops.mlp_block_fwd(n.to(t).cuda(), gin.cuda() if affine else None, bin_.cuda() if affine else None, W1.to(t).cuda(),
                            b1.cuda(), W2.to(t).cuda(), b2.cuda(), torch.ones(E).cuda(), torch.zeros(E).cuda(), act=1, extras=True)
    torch.cuda.synchronize()
    for k, r in (("u", u), ("h", h), ("z", z)):
        assert torch.equal(out[k].float().cpu(), r), k


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_attn_block_fwd_folded_affine_exact(w, dt):
    """Zero q / k weights -> uniform probabilities 1/32 (S = 32); v = (gamma n + beta) Wv^T + bv with gamma in {0.5, 1, 2} and
    small-integer beta is exact, and so are ctx (a mean of 32 of them), the out-projection and the residual."""
    from moleculardiffusion_mivit_amd import ops
    E, _, _ = WIDTHS[w]
    B, S = 5, 32
    n = _ints((B, S, E), 5, 2, 5, 1)
    gin = torch.tensor([0.5, 1.0, 2.0])[(torch.arange(E) * 5 + 2) % 3]
    bin_ = _ints((E,), 3, 1, 1, 0)
    idx = torch.arange(E)
    Wqkv = torch.zeros(3 * E, E)
    Wqkv[2 * E + idx, (idx * 37 + 5) % E] = 1.0
    Wqkv[2 * E + idx, (idx * 11 + 3) % E] += 2.0
    bqkv = torch.zeros(3 * E)
    bqkv[2 * E:] = _ints((E,), 5, 2, 3, 0)
    Wo = torch.zeros(E, E)
    Wo[idx, (idx * 13 + 7) % E] = 1.0
    bo = _ints((E,), 3, 1, 2, 0)
    x = gin * n + bin_
    v = x @ Wqkv[2 * E:].t() + bqkv[2 * E:]
    ctx = v.mean(dim=1, keepdim=True).expand(B, S, E)
    z = x + ctx @ Wo.t() + bo
    for t_ in (v, ctx):
        assert torch.equal(t_.to(torch.bfloat16).float(), t_)            # exact in bf16 (and so in fp16)
    t = DT[dt]
    out = ops.attn_block_fwd(n.to(t).cuda(), gin.cuda(), bin_.cuda(), Wqkv.to(t).cuda(), bqkv.cuda(), Wo.to(t).cuda(), bo.cuda(),
                             torch.ones(E).cuda(), torch.zeros(E).cuda(), extras=True)
    torch.cuda.synchronize()
    assert torch.equal(out["qkv"].float().cpu()[..., 2 * E:], v)
    assert torch.equal(out["ctx"].float().cpu(), ctx)
    assert torch.equal(out["z"].float().cpu(), z.to(t).float())


@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("fix", [False, True])
def test_qkv_bwd_exact(w, dt, fix):
    """Small integers, and with the fix-up gamma in {0.5, 1, 2} and small-integer beta: dx, dW, db are exact (fp32 holds every
    partial sum), so the fix-up applying gamma or beta of another column is an exact mismatch."""
    from moleculardiffusion_mivit_amd import ops
    E, _, _ = WIDTHS[w]
    M = 2777
    dqkv = _ints((M, 3 * E), 5, 2, 7, 3)
    x = _ints((M, E), 3, 1, 11, 1)
    W = _sparse((3 * E, E), 31, 13, 5, 3)
    res = _ints((M, E), 7, 3, 3, 2)
    g = torch.tensor([0.5, 1.0, 2.0])[(torch.arange(E) * 7 + 2) % 3] if fix else None
    b = _ints((E,), 5, 2, 3, 1) if fix else None
    ref, _ = qkv_bwd_ref(dqkv.double(), x.double(), W.double(), res.double(), None if g is None else g.double(),
                         None if b is None else b.double())
    assert float(ref["dx"].abs().max()) <= 256
    t = DT[dt]
    out = ops.qkv_bwd(dqkv.to(t).cuda(), x.to(t).cuda(), W.to(t).cuda(), res.to(t).cuda(),
                      fix_gamma=None if g is None else g.cuda(), fix_beta=None if b is None else b.cuda())
    torch.cuda.synchronize()
    for k in ("dx", "dW", "db"):
        assert torch.equal(out[k].double().cpu(), ref[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# GPU: placement -- NaN-filled outputs with sentinel guard rows, raw C-ABI, ragged bench-scale M
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", [128, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("extras", [False, True])
def test_placement(w, dt, extras):
    """Every in-range element of every output is written (finite), no guard element behind an output changes.  An unwritten
    row of `u` (torch.empty outputs) or a store past the last row fails here deterministically."""
    E, F, _ = WIDTHS[w]
    t = DT[dt]
    M = BENCH_M
    f32 = torch.float32
    # mlp_block_fwd
    p = _cuda(mlp_fwd_inputs(M, w, dt, True, _seed("pl-mf", w, dt)))
    bufs = {"n": _guarded(M, E, t), "rstd": _guarded(M, 0, f32)}
    if extras:
        bufs.update(x=_guarded(M, E, t), z=_guarded(M, E, t), mean=_guarded(M, 0, f32), h=_guarded(M, F, t), u=_guarded(M, F, t))
    o = lambda k: _p(bufs[k][1]) if k in bufs else _p(None)
    _call("mivit_mlp_block_fwd", w, dt, *[_p(p[k]) for k in ("n", "gin", "bin", "W1", "b1", "W2", "b2", "gout", "bout")], M, 3,
          o("n"), o("rstd"), o("x"), o("z"), o("mean"), o("h"), o("u"), _stream())
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        _check_guarded(f"mlp_block_fwd {k}", buf, M)
    # attn_block_fwd: 4133 sequences of 33 tokens
    B, S = 4133, 33
    a = _cuda(attn_fwd_inputs(B, S, w, dt, True, _seed("pl-af", w, dt)))
    R = B * S
    bufs = {"ctx": _guarded(R, E, t), "n": _guarded(R, E, t), "rstd": _guarded(R, 0, f32)}
    if extras:
        bufs.update(x=_guarded(R, E, t), z=_guarded(R, E, t), mean=_guarded(R, 0, f32), qkv=_guarded(R, 3 * E, t))
    o = lambda k: _p(bufs[k][1]) if k in bufs else _p(None)
    _call("mivit_attn_block_fwd", w, dt, *[_p(a[k]) for k in ("n", "gin", "bin", "Wqkv", "bqkv", "Wo", "bo", "gout", "bout")], B, S,
          o("ctx"), o("n"), o("rstd"), o("x"), o("z"), o("mean"), o("qkv"), _stream())
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        _check_guarded(f"attn_block_fwd {k}", buf, R)
    if extras:          # the backward blocks have no optional outputs: run them once
        return
    # mlp_block_bwd
    q = _cuda(mlp_bwd_inputs(M, w, dt, _seed("pl-mb", w, dt)))
    dx1 = _guarded(M, E, t)
    grads = {k: _guarded(n, 0, f32) for k, n in (("dW1", F * E), ("db1", F), ("dW2", E * F), ("db2", E), ("dgamma2", E), ("dbeta2", E))}
    nb = _entry("mivit_mlp_block_bwd_workspace_bytes", w, dt)(M)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    _call("mivit_mlp_block_bwd", w, dt, *[_p(q[k]) for k in ("dy", "n2", "rstd2", "gamma2", "n1", "gamma1", "beta1", "W1", "b1", "W2")],
          M, 1, _p(dx1[1]), *[_p(g[1]) for g in grads.values()], _p(ws), nb, _stream())
    torch.cuda.synchronize()
    _check_guarded("mlp_block_bwd dx1", dx1[0], M)
    for k, (buf, v) in grads.items():
        _check_guarded(f"mlp_block_bwd {k}", buf, v.shape[0])
    # attn_out_bwd
    r = _cuda(attn_out_bwd_inputs(M, w, dt, _seed("pl-ao", w, dt)))
    dz1, dctx = _guarded(M, E, t), _guarded(M, E, t)
    grads = {k: _guarded(n, 0, f32) for k, n in (("dWo", E * E), ("dbo", E), ("dgamma1", E), ("dbeta1", E))}
    nb = _entry("mivit_attn_out_bwd_workspace_bytes", w, dt)(M)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    _call("mivit_attn_out_bwd", w, dt, *[_p(r[k]) for k in ("dy", "n1", "rstd1", "gamma1", "ctx", "Wo")], M, _p(dz1[1]), _p(dctx[1]),
          *[_p(g[1]) for g in grads.values()], _p(ws), nb, _stream())
    torch.cuda.synchronize()
    _check_guarded("attn_out_bwd dz1", dz1[0], M)
    _check_guarded("attn_out_bwd dctx", dctx[0], M)
    for k, (buf, v) in grads.items():
        _check_guarded(f"attn_out_bwd {k}", buf, v.shape[0])
    # qkv_bwd (with the fix-up)
    qv = _cuda(qkv_bwd_inputs(M, w, dt, True, _seed("pl-qb", w, dt)))
    dx = _guarded(M, E, t)
    dW, db = _guarded(3 * E * E, 0, f32), _guarded(3 * E, 0, f32)
    nb = _entry("mivit_qkv_bwd_workspace_bytes", w, dt)(M)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    _call("mivit_qkv_bwd_affine", w, dt, *[_p(qv[k]) for k in ("dqkv", "x", "Wqkv", "res")], M, _p(dx[1]), _p(dW[1]), _p(db[1]),
          _p(qv["fix_gamma"]), _p(qv["fix_beta"]), _p(ws), nb, _stream())
    torch.cuda.synchronize()
    _check_guarded("qkv_bwd dx", dx[0], M)
    _check_guarded("qkv_bwd dW", dW[0], 3 * E * E)
    _check_guarded("qkv_bwd db", db[0], 3 * E)
