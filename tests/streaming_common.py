"""References, dispatch restatements and case tables of tests/test_streaming_ops.py (CPU) and tests/test_streaming_ops_gpu.py:
the streaming GEMM family -- csrc/rowstream.hip, wavestream.hip, gemm_dma.hip, wgrad_dma.hip, wgrad_small.hip and the frame
embedding launches of csrc/embed.hip -- called through the operator level of the C-ABI in bf16 and, through the _f16 entries,
in IEEE half.  Plain torch on the CPU; importing this module needs no GPU.

Rounding model, read from the kernels (`rnd` = round-to-nearest-even to the element type T, `acc` = the fp32 MFMA sum):
  * bias.  Added in fp32 to the accumulator before anything else: rowstream.hip:234 (`acc + bias_v` into the fp32 staging
    tile), wavestream.hip:177, gemm_dma.hip:194 (launch_t kernels) and :353 (transposed-product kernels).  Never in 16 bits.
  * y_preact = rnd(acc + bias): rowstream.hip:245, wavestream.hip:189, gemm_dma.hip:206 / :356 -- stored with y's stride.
  * activation: on the UNROUNDED fp32 value acc + bias (rowstream.hip:247, wavestream.hip:191, gemm_dma.hip:208 / :358), then
    the residual (widened to fp32) is added and y = rnd(act(acc + bias) + resid) is the only rounding (rowstream.hip:252-254,
    wavestream.hip:196-198, gemm_dma.hip:213 / :229, :363 / :379).  That is gemm.hip's model: operators_common.ref_linear_fwd.
  * dgrad: dx = rnd(acc * act'(saved) + dres), all in fp32; act' from common.h:80-90 (relu / leaky test `saved > 0` strictly,
    gelu' takes the pre-activation).  The row- and wave-stream kernels take ONE epilogue operand (saved or dres:
    rowstream.hip:344, wavestream.hip:286); gemm_dma takes both (gemm_dma.hip:216-227, :366-377).
  * fused LayerNorm: normalises the ROUNDED sum, z = rnd(y) widened again (rowstream.hip:261, wavestream.hip:202): mean =
    sum / N, variance two-pass and biased, rstd = rsqrtf(var + 1e-5), ln_out = rnd((z - mean) * rstd * gamma + beta) (:266-277,
    :209-224); mean / rstd fp32.  ln_out is stored with stride N (the C entries pass ldy = N: rowstream.hip:375,
    wavestream.hip:352), so its padding cannot be set through the C-ABI.  The tests feed the reference LayerNorm the z the
    kernel stored (itself held to its own bar): the two halves are judged independently.
  * fp32 frames: rounded to T (RNE) when staged -- wavestream.hip:146 (`(__bf16)` of the fp32 pixel), wgrad_small.hip:105
    (store16 of the fp32 pixels), embed.hip cvt8 -- and multiplied as T; pixels past the row length are zeroed in registers.
  * weight gradients: dW = dy^T x and db = column sums of dy, fp32 accumulators per row split, splits summed in a fixed order
    (wgrad_dma.hip:220-222, wgrad_small.hip:125-164, :231-232): bitwise repeatable.
NULL bias is allowed everywhere (`if (a.bias)`: rowstream.hip:141, wavestream.hip:109, gemm_dma.hip:185 / :342); db == NULL
skips the column sums (wgrad_dma.hip:196, wgrad_small.hip:218 / :249).

Not reachable through the C-ABI: a strided W (ldw = K always), ln_out's stride, the MIVIT_XCD_REMAP=0 dispatch order, the
engine-only row-stream launches with a strided ln_out, MIVIT_EMBED_WGRAD_CFG = 2 and MIVIT_EMBED_WGRAD_VARIANT (environment reads).
"""
import torch

import operators_common as oc
from operators_common import cdiv

H16 = ("bf16", "f16")
INT_LIMIT = {"bf16": 256.0, "f16": 2048.0}


def _c(**kw):
    return kw


# ---------------------------------------------------------------------------------------------------------------------
# dispatch restatements.  Shapes are the GEMM's own: out columns NC, contraction KC (forward: NC = N, KC = K; dgrad: NC = K, KC = N)
# ---------------------------------------------------------------------------------------------------------------------
def gemm_dims(c):
    return (c["K"], c["N"]) if c["kind"] == "dgrad" else (c["N"], c["K"])


def rowstream_supported(M, NC, KC, dgrad, lda=8, a_off=0):
    """rowstream.hip:312-318"""
    if not (KC in (128, 256) or (KC == 384 and dgrad)) or NC % 128 or M < 256:
        return False
    return lda % 8 == 0 and (a_off * 2) % 16 == 0


def wavestream_supported(M, NC, KC, dgrad, lda=8, a_off=0):
    """wavestream.hip:264-273"""
    if not (KC in (64, 128, 256) or (KC == 192 and dgrad and NC == 64)) or NC % 64 or M < 256:
        return False
    if KC == 256 and NC % 128:
        return False
    return lda % 8 == 0 and (a_off * 2) % 16 == 0


def ws_pick(mode, mask, NC, KC, dgrad, ln, dact):
    """launch_rowstream's choice (rowstream.hip:328-336), before wavestream_supported is asked"""
    rs_shape = (KC in (128, 256) or (KC == 384 and dgrad)) and NC % 128 == 0
    return (not rs_shape) or mode == 1 or (mode == 2 and bool(((mask & 1) and KC == 128 and not dgrad and ln) or
                                                             ((mask & 2) and KC == 128 and dgrad and dact) or
                                                             ((mask & 4) and KC == 256 and dgrad)))


def epi_kind(dgrad, ln, dact, resid):
    """E_KIND of RS_GO / ws_dispatch: 0 none, 1 forward residual, 2 act'(saved), 3 residual gradient"""
    if dgrad:
        return 2 if dact else 3 if resid else 0
    return 1 if (ln or resid) else 0


def rs_instance(NC, KC, dgrad, ln, dact, resid):
    """RS_GO (rowstream.hip:349-361): rs_launch<K, DGRAD, LN, E_KIND>"""
    return ("rs", KC, dgrad, bool(ln), epi_kind(dgrad, ln, dact, resid))


def ws_instance(NC, KC, dgrad, ln, dact, resid):
    """launch_wavestream / ws_dispatch (wavestream.hip:249-304): ws_launch<K, BN, DGRAD, LN, E_KIND>"""
    return ("ws", KC, 128 if NC % 128 == 0 else 64, dgrad, bool(ln), epi_kind(dgrad, ln, dact, resid))


def rs_cfg(KC, dgrad, has_e):
    """RsCfg (rowstream.hip:40-60): (BM, ring slots, LDS bytes)"""
    BM = 32 if KC > 256 else 64
    slot = BM * 2 * KC + (BM * 128 * 2 if has_e else 0)
    w = (KC if dgrad else 128) * (256 if dgrad else 2 * KC)
    ns = 3 if w + 3 * slot <= 160 * 1024 else 2
    return BM, ns, w + ns * slot


def rs_grid_y(M, NC, KC, dgrad, has_e):
    """rs_launch (rowstream.hip:292-296): row walkers; a walker takes a second tile when ceil(M / BM) exceeds it"""
    BM, _, lds = rs_cfg(KC, dgrad, has_e)
    return max(1, min(256 * (2 if lds <= 80 * 1024 else 1) // (NC // 128), cdiv(M, BM))), BM


def ws_nwv(KC):
    return 16 if KC == 64 else 12 if KC == 128 else 8


def ws_grid_y(M, NC, KC):
    """ws_launch (wavestream.hip:237-240): a wave takes a second 16-row tile when ceil(M / 16) exceeds gy * NWV"""
    ntn = NC // (128 if NC % 128 == 0 else 64)
    return max(1, min(256 // ntn, cdiv(cdiv(M, 16), ws_nwv(KC))))


def frame_kp(K):
    """wavestream.hip:307 / wgrad_small.hip:196 (frame_kb is the same ladder)"""
    for kp in (64, 96, 128, 192, 256):
        if K <= kp:
            return kp
    return 0


frame_kb = frame_kp


def frame_nb(N, K):
    kb = frame_kb(K)
    if not kb or N not in (64, 128):
        return 0
    return 64 if kb <= 96 else 32


def window_of(N, K):
    """wgrad_small.hip:187-192"""
    if K == 64 and N in (64, 128):
        return N
    if K == 64 and N == 192:
        return 96
    if K == 128 and N == 64:
        return 64
    return 0


def embed_small_supported(M, K, E):
    return frame_kp(K) != 0 and E in (64, 128) and M >= 256 and M * K * 4 < 2 ** 32


def small_grid_x(M, nsplit, NW=8):
    """wgrad_small.hip launch_t: workgroups per column window (1 = in place, no slabs)"""
    nchunks = cdiv(M, 32)
    return 1 if nchunks <= 32 else max(1, min(256 // nsplit, cdiv(nchunks, NW)))


def small_ws_bytes(N, K):
    return cdiv(256 * N * (K + 1) * 4, 256) * 256


def gemm_dma_supported(M, NC, KC):
    return M >= 256 and NC % 128 == 0 and KC % 64 == 0 and KC >= 128


_GD_BIG = {0: (2, 2, 8, 4), 1: (4, 1, 4, 3), 2: (2, 2, 4, 3), 3: (8, 1, 2, 3), 7: (4, 2, 4, 3)}       # WM, WN, TM, NS
_GD_T = {1: (64, 32, 3, 4), 2: (64, 32, 4, 4), 3: (64, 64, 2, 4), 4: (32, 64, 3, 4), 5: (32, 64, 2, 4), 6: (32, 32, 3, 8),
         7: (32, 32, 2, 8), 8: (32, 64, 2, 8), 9: (32, 32, 3, 4), 10: (64, 32, 2, 4), 11: (64, 32, 2, 8)}   # BMW, BK, NS, NW
GD_VARIANTS = list(range(0, 12)) + [19, 20, 21, 22, 23, 27, 30, 31, 32, 33, 37]


def gemm_dma_instance(variant, M, NC, dgrad):
    """launch_variant (gemm_dma.hip:532-569)"""
    if variant >= 20 and M >= 256 and variant // 10 in (2, 3) and variant % 10 in _GD_BIG:
        cfg = _GD_BIG[variant % 10]
        if cfg[1] == 1 or NC % 256 == 0:
            return ("gd-pers" if variant >= 30 else "gd-big",) + cfg + (dgrad,)
    if variant in _GD_T:
        return ("gd-t",) + _GD_T[variant] + (dgrad,)
    return ("gd-t", 32, 32, 2 if dgrad else 3, 8, dgrad)


def gemm_pers_grid(M, NC, cfg):
    """launch_pers (gemm_dma.hip:514-524): (tiles, workgroups); a workgroup takes a second tile when tiles > workgroups"""
    WM, WN, TM, NS = cfg
    BM, BN = WM * TM * 16, WN * 128
    bytes_ = NS * (BM * 64 + BN * 64)
    minb = max(1, (8 if TM <= 4 else 4) // (WM * WN))
    per_cu = max(1, min(160 * 1024 // bytes_, minb))
    ntile = cdiv(cdiv(M, BM), 8) * 8 * (NC // BN)
    return ntile, min(ntile, 256 * per_cu)


def wgrad_dma_splits(M, N, K):
    """dma_splits + the rounding of launch_wgrad_dma (wgrad_dma.hip:165-172, :192-195) -> (splits asked, slabs launched)"""
    tiles = (N // 128) * (K // 128)
    s = max(1, min(cdiv(512, tiles), cdiv(M, 128)))
    rps = cdiv(cdiv(M, s), 64) * 64
    return s, cdiv(M, rps)


def wgrad_dma_ws_bytes(M, N, K):
    return cdiv(wgrad_dma_splits(M, N, K)[0] * N * (K + 1) * 4, 256) * 256


def wgrad_dma_config(cfg, N, K):
    """launch_wgrad_dma (wgrad_dma.hip:204-213): (ring slots, rows per stage)"""
    cfg = cfg or (21 if N * K >= 512 * 512 else 22)
    return {32: (3, 64), 21: (2, 32), 31: (3, 32)}.get(cfg, (2, 64))


def embed_dma_supported(M, K, E):
    return E % 128 == 0 and K % 128 == 0 and K >= 256 and M >= 128


EMBED_VARIANTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 15]


def embed_fwd_instance(variant, M, E):
    """launch_embed_fwd_dma (embed.hip:747-772)"""
    t = {2: ("dma", 128, 3), 1: ("dma", 256, 2), 3: ("direct", 2, 4, 3), 14: ("direct2", 2, 4, 3), 4: ("direct", 1, 4, 2),
         5: ("direct", 1, 8, 3), 6: ("direct", 1, 8, 2), 7: ("direct", 2, 4, 2), 8: ("direct", 1, 4, 3), 15: ("direct", 1, 2, 3),
         13: ("dma32",)}
    if variant in t:
        return t[variant]
    if cdiv(M, 128) * (E // 128) >= 512:
        return ("direct2", 2, 4, 3)
    if cdiv(M, 64) * (E // 128) >= 512:
        return ("direct", 1, 4, 3)
    return ("direct", 1, 2, 3)


def embed_wgrad_ws_bytes(M, K, E):
    tiles = (K // (256 if K % 256 == 0 else 128)) * max(1, E // 128)
    return max(1, min(cdiv(512, tiles), cdiv(M, 512))) * E * K * 4


def case_instance(c, dt, mask=7):
    """the kernel template instantiation a forward / dgrad case runs, under its own setter state"""
    NC, KC = gemm_dims(c)
    dg = c["kind"] == "dgrad"
    ln, dact, resid = bool(c.get("ln")), bool(c.get("dact")), bool(c.get("resid"))
    if c["fam"] == "gemm_dma":
        return gemm_dma_instance(c.get("variant", 0), c["M"], NC, dg)
    if c["fam"] == "wavestream":
        return ws_instance(NC, KC, dg, ln, dact, resid)
    if ws_pick(c.get("ws_mode", 2), mask, NC, KC, dg, ln, dact) and wavestream_supported(c["M"], NC, KC, dg):
        return ws_instance(NC, KC, dg, ln, dact, resid)
    return rs_instance(NC, KC, dg, ln, dact, resid)


# ---------------------------------------------------------------------------------------------------------------------
# references (fp64 by default; cdt = float32 is the restatement behind the yardsticks)
# ---------------------------------------------------------------------------------------------------------------------
ref_fwd = oc.ref_linear_fwd                  # (dt, x, W, bias, act, resid) -> (y, y_preact) unrounded: the model above is gemm.hip's
ref_dgrad = oc.ref_linear_dgrad              # (dt, dy, W, act, saved, dres) -> dx unrounded
ref_ln = oc.ref_ln_fwd                       # (z, gamma, beta) on the STORED z -> (ln_out unrounded, mean, rstd)


def ref_wgrad(dt, dy, x, cdt=torch.float64):
    """dy: values of T; x: values of T, or the fp32 frames (rounded to T when staged) -> (dW, db)"""
    return dy.to(cdt).t() @ oc.rnd(x, dt).to(cdt), dy.to(cdt).sum(0)


def autograd_check(dt, x, W, bias, act, resid, dy):
    """the references against torch autograd in fp64 on h = act(x W^T + b), y2 = h W2^T: forward (with the residual), the
    data gradient with act'(saved) fused, the plain data gradient and the weight gradient -> worst differences"""
    xr = oc.rnd(x, dt).double().requires_grad_()
    Wr = oc.rnd(W, dt).double().requires_grad_()
    b = bias.double().requires_grad_()
    W2 = oc.randn((16, W.shape[0]), 9, 0.2, dt)
    u = xr @ Wr.t() + b
    u.retain_grad()
    h = {0: lambda t: t, 1: torch.relu, 2: lambda t: torch.nn.functional.leaky_relu(t, 0.01),
         3: lambda t: torch.nn.functional.gelu(t)}[act](u)
    dy2 = dy[:, :16]
    (h @ W2.double().t()).backward(dy2.double())
    saved = u.detach() if act == 3 else h.detach()
    du = ref_dgrad(dt, dy2, W2, act, saved, None)
    dx = ref_dgrad(dt, du, W, 0, None, None)
    dW, db = ref_wgrad(dt, du, x)
    y_ref, u_ref = ref_fwd(dt, x, W, bias, act, resid)
    return (float((y_ref - (h.detach() + resid.double())).abs().max()), float((u_ref - u.detach()).abs().max()),
            float((du - u.grad).abs().max()), float((dx - xr.grad).abs().max()), float((dW - Wr.grad).abs().max()),
            float((db - b.grad).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# operands: small integers whose every intermediate is exact (checked by tests/test_streaming_ops.py)
# ---------------------------------------------------------------------------------------------------------------------
def int_operands(c):
    """-> dict of fp32 tensors for a forward / dgrad / wgrad / embedding case"""
    M, N, K = c["M"], c["N"], c["K"]
    kind = c["kind"]
    o = {}
    if kind == "fwd":
        o["x"] = oc.ints((M, K), 7, 3, 5, -2, 1)
        o["W"] = oc.ints((N, K), 5, 11, 7, -3, 1).sign() * (oc.ints((N, K), 3, 1, 4, 0) > 0)         # {-1, 0, 1}
        o["bias"] = None if c.get("nobias") else oc.ints((N,), 3, 0, 9, -4)
        if c.get("resid") or c.get("ln"):
            o["resid"] = oc.ints((M, N), 5, 7, 13, -6, 1)
        if c.get("ln"):
            o["gamma"] = 1 + 0.25 * oc.ints((N,), 3, 0, 5, -2)
            o["beta"] = 0.5 * oc.ints((N,), 5, 0, 7, -3)
    elif kind == "dgrad":
        o["dy"] = oc.ints((M, N), 7, 3, 5, -2, 1)
        o["W"] = oc.ints((N, K), 5, 11, 7, -3, 1).sign() * (oc.ints((N, K), 3, 1, 4, 0) > 0)
        if c.get("dact"):
            o["saved"] = oc.ints((M, K), 3, 5, 7, -3, 1)                                              # negative, zero, positive
        if c.get("resid"):
            o["dres"] = oc.ints((M, K), 5, 7, 13, -6, 1)
    else:                                                                                             # wgrad / embed_*: x [M, K]
        o["dy"] = oc.ints((M, N), 7, 3, 5, -2, 1)
        o["x"] = oc.ints((M, K), 5, 11, 7, -3, 1) if kind == "wgrad" else oc.ints((M, K), 3, 7, 5, -2, 2)
        o["W"] = oc.ints((N, K), 5, 11, 7, -3, 1).sign() * (oc.ints((N, K), 3, 1, 4, 0) > 0)
        o["bias"] = oc.ints((N,), 3, 0, 9, -4)
    return o


def rand_operands(c, dt, seed=0):
    """|x| ~ 1, the contraction scaled so that outputs are ~ 1 too; 16-bit operands already rounded to T"""
    M, N, K = c["M"], c["N"], c["K"]
    kind = c["kind"]
    r = lambda shape, i, scale=1.0, d=dt: oc.randn(shape, seed * 16 + i, scale, d)
    o = {}
    if kind == "fwd":
        o.update(x=r((M, K), 1), W=r((N, K), 2, K ** -0.5), bias=None if c.get("nobias") else r((N,), 3, 1.0, None))
        if c.get("resid") or c.get("ln"):
            o["resid"] = r((M, N), 4)
        if c.get("ln"):
            o["gamma"] = 1 + 0.1 * r((N,), 5, 1.0, None)
            o["beta"] = 0.1 * r((N,), 6, 1.0, None)
    elif kind == "dgrad":
        o.update(dy=r((M, N), 1), W=r((N, K), 2, N ** -0.5))
        if c.get("dact"):
            o["saved"] = r((M, K), 3)
        if c.get("resid"):
            o["dres"] = r((M, K), 4)
    else:
        o.update(dy=r((M, N), 1), x=r((M, K), 2, 1.0, None if c["fam"].startswith("embed") else dt), W=r((N, K), 3, K ** -0.5),
                 bias=r((N,), 4, 1.0, None))
    return o


# ---------------------------------------------------------------------------------------------------------------------
# case tables.  Forward (M, N, K): x [M, K] ldx, W [N, K], y / y_preact [M, N] ldy, resid ldr.  Dgrad (M, N, K): dy [M, N] lddy,
# W [N, K], saved / dres / dx [M, K].  Every ld is width + pad (pad 8 or 24), every base pointer `off` = 8 elements (16 bytes)
# into its allocation.  act / dact: 0 none, 1 relu, 2 leaky, 3 gelu.  ws_mode: the mivit_rowstream_set_wavestream state.
# ---------------------------------------------------------------------------------------------------------------------
WAVE_M = (256, 257, 271)              # 16-row wave tiles
RING_M = (256, 257, 319)              # 64- / 32-row ring tiles
GD_M = (256, 257, 511)                # 256-row gemm_dma tiles
WS_SHAPES = [(64, 128), (128, 128), (256, 128), (64, 64), (128, 64)]                 # (contraction, BN)
EPIS_FWD = [dict(), dict(resid=True, act=1, pre=True), dict(ln=True), dict(act=1, pre=True, nobias=True)]
EPIS_DGRAD = [dict(), dict(dact=1), dict(resid=True)]


def _mk(fam, kind, M, NC, KC, i, **kw):
    N, K = (KC, NC) if kind == "dgrad" else (NC, KC)
    name = "-".join(f"{k}{'' if v is True else v}" for k, v in kw.items()) or "plain"
    return _c(id=f"{fam}-{kind}-{M}x{N}x{K}-{name}", fam=fam, kind=kind, M=M, N=N, K=K, pad=(8, 24)[i % 2], off=8, **kw)


def _family_cases():
    out, i = [], 0
    # wave-stream: every (K, BN) x epilogue; one column tile (fused LayerNorm needs N == BN), and several for the rest
    for KC, BN in WS_SHAPES:
        for e in EPIS_FWD:
            NC = BN if (e.get("ln") or i % 2) else 3 * BN if BN == 64 else 2 * BN
            out.append(_mk("wavestream", "fwd", WAVE_M[i % 3], NC, KC, i, **e)); i += 1
        for e in EPIS_DGRAD:
            NC = BN if i % 2 else 3 * BN if BN == 64 else 2 * BN
            out.append(_mk("wavestream", "dgrad", WAVE_M[i % 3], NC, KC, i, **e)); i += 1
    for e in EPIS_DGRAD:                                       # the q|k|v data gradient of the 64-wide models
        out.append(_mk("wavestream", "dgrad", WAVE_M[i % 3], 64, 192, i, **e)); i += 1
    # row-stream entry: K in {128, 256} (+ 384 dgrad), one column tile and several; under setter mode 0 (the DMA-ring kernels
    # themselves), 1 (always wave-stream where it supports the shape) and 2 (the default picks)
    for mode in (0, 1, 2):
        for KC in (128, 256):
            for NC in (128, 256 if KC == 128 else 384):
                for e in EPIS_FWD:
                    if e.get("ln") and NC != 128:
                        continue
                    out.append(_mk("rowstream", "fwd", RING_M[i % 3], NC, KC, i, ws_mode=mode, **e)); i += 1
        for KC in (128, 256, 384):
            for NC in (128, 256):
                for e in EPIS_DGRAD:
                    out.append(_mk("rowstream", "dgrad", RING_M[i % 3], NC, KC, i, ws_mode=mode, **e)); i += 1
    # gemm_dma: every variant, forward with everything fused and dgrad with saved AND dres
    for v in GD_VARIANTS:
        out.append(_mk("gemm_dma", "fwd", GD_M[i % 3], 256, 256, i, variant=v, resid=True, act=1, pre=True)); i += 1
        out.append(_mk("gemm_dma", "dgrad", GD_M[i % 3], 256, 256, i, variant=v, dact=1, resid=True)); i += 1
    out.append(_mk("gemm_dma", "fwd", 257, 384, 192, i, variant=0, nobias=True)); i += 1
    out.append(_mk("gemm_dma", "dgrad", 511, 128, 320, i, variant=0)); i += 1
    # one M per kernel just past the point where a workgroup / wave takes a second tile (rs_grid_y, ws_grid_y, gemm_pers_grid)
    out.append(_mk("wavestream", "fwd", 4096 + 17, 1024, 256, i, resid=True, act=1)); i += 1
    out.append(_mk("rowstream", "fwd", 4096 + 65, 1024, 128, i, ws_mode=0, resid=True, act=1)); i += 1
    out.append(_mk("rowstream", "dgrad", 2048 + 33, 1024, 384, i, ws_mode=0, dact=1)); i += 1
    out.append(_mk("gemm_dma", "fwd", 8192 + 257, 1024, 128, i, variant=33, act=1)); i += 1
    return out


FAMILY_CASES = _family_cases()

# accuracy: random operands.  leaky / gelu forward, leaky' / gelu' backward, activation + residual, y_preact + residual
_ACC = []
for _i, (_fam, _KC, _NC, _M, _mode) in enumerate([("wavestream", 64, 128, 257, None), ("wavestream", 128, 64, 271, None),
                                                    ("wavestream", 256, 256, 257, None), ("rowstream", 128, 256, 319, 0),
                                                    ("rowstream", 256, 128, 257, 0), ("gemm_dma", 256, 256, 511, None)]):
    _kw = {} if _mode is None else dict(ws_mode=_mode)
    for _e in (dict(act=2, resid=True, pre=True), dict(act=3, resid=True, pre=True), dict(act=3), dict(act=0, nobias=True)):
        _ACC.append(_mk(_fam, "fwd", _M, _NC, _KC, _i, **_kw, **_e))
    if _NC in (64, 128):
        _ACC.append(_mk(_fam, "fwd", _M, _NC, _KC, _i, ln=True, act=0, **_kw))
    for _e in (dict(dact=2), dict(dact=3), dict(resid=True)) + ((dict(dact=3, resid=True),) if _fam == "gemm_dma" else ()):
        _ACC.append(_mk(_fam, "dgrad", _M, _NC, _KC, _i, **_kw, **_e))
_ACC.append(_mk("rowstream", "dgrad", 319, 128, 384, 0, ws_mode=0, dact=3))
_ACC.append(_mk("wavestream", "dgrad", 271, 64, 192, 1, dact=2))
_ACC.append(_mk("gemm_dma", "fwd", 257, 256, 256, 0, variant=21, act=3, resid=True, pre=True))
_ACC.append(_mk("gemm_dma", "dgrad", 257, 256, 256, 1, variant=31, dact=3, resid=True))
ACCURACY_CASES = _ACC


def _wg(fam, M, N, K, i, **kw):
    name = "-".join(f"{k}{'' if v is True else v}" for k, v in kw.items()) or "plain"
    return _c(id=f"{fam}-{M}x{N}x{K}-{name}", fam=fam, kind="wgrad", M=M, N=N, K=K, pad=(8, 24)[i % 2], off=8, **kw)


# weight gradients: dy [M, N] lddy, x [M, K] ldx -> dW [N, K], db [N]
WGRAD_CASES = (
    [_wg("wgrad_bf16", RING_M[i % 3], N, K, i, cfg=cfg, **({"nodb": True} if i % 4 == 3 else {}))
     for i, (cfg, N, K) in enumerate([(0, 128, 128), (0, 512, 512), (21, 128, 256), (22, 256, 128), (31, 128, 128),
                                      (32, 128, 128), (31, 256, 128), (32, 128, 256)])]
    + [_wg("wgrad_bf16", 1000 + 7, 128, 128, 0, cfg=0), _wg("wgrad_bf16", 700 + 1, 128, 128, 1, cfg=32)]
    + [_wg("wgrad_small", WAVE_M[i % 3], N, K, i, **({"nodb": True} if i == 1 else {}))
       for i, (N, K) in enumerate([(64, 64), (128, 64), (192, 64), (64, 128)])]
    + [_wg("wgrad_small", 1024 + 33, 192, 64, 0),                        # slabs: more than 32 chunks
       _wg("wgrad_small", 32768 + 33, 192, 64, 1)]                       # a wave takes a second chunk (small_grid_x)
)
SMALL_K, SMALL_E = (25, 81, 96, 121, 169, 225, 256), (64, 128)
EMBED_SMALL_CASES = (
    [_c(id=f"embed_small-257x{E}x{K}", fam="embed_small", kind="embed", M=257, N=E, K=K, off=1) for K in SMALL_K for E in SMALL_E]
    + [_c(id="embed_small-slabs-1057x64x81", fam="embed_small", kind="embed", M=1057, N=64, K=81, off=1),
       _c(id="embed_small-second-chunk-8225x128x256", fam="embed_small", kind="embed", M=8225, N=128, K=256, off=0, wgrad_only=True),
       _c(id="embed_small-second-tile-32785x128x256", fam="embed_small", kind="embed", M=32785, N=128, K=256, off=0, fwd_only=True)]
)
EMBED_LARGE_CASES = [_c(id=f"embed_large-v{v}", fam="embed_large", kind="embed", M=128, N=128, K=256, variant=v)
                     for v in EMBED_VARIANTS] + [_c(id="embed_large-ragged-v0", fam="embed_large", kind="embed", M=131, N=128,
                                                    K=384, variant=0)]

# what the tables must reach, in both element types (gemm_dma: bf16 only) -- asserted by tests/test_streaming_ops.py
REQUIRED_WS = ({("ws", KC, BN, False, False, ek) for KC, BN in WS_SHAPES for ek in (0, 1)}
               | {("ws", KC, BN, False, True, 1) for KC, BN in WS_SHAPES}
               | {("ws", KC, BN, True, False, ek) for KC, BN in WS_SHAPES + [(192, 64)] for ek in (0, 2, 3)})
REQUIRED_RS = ({("rs", KC, False, False, ek) for KC in (128, 256) for ek in (0, 1)} | {("rs", KC, False, True, 1) for KC in (128, 256)}
               | {("rs", KC, True, False, ek) for KC in (128, 256, 384) for ek in (0, 2, 3)})
RS_BEHIND_PICKS = {("rs", 128, False, True, 1), ("rs", 128, True, False, 2), ("rs", 256, True, False, 0),
                   ("rs", 256, True, False, 2), ("rs", 256, True, False, 3)}
REQUIRED_GD = {gemm_dma_instance(v, 256, 256, dg) for v in GD_VARIANTS for dg in (False, True)}


def case_dts(c):
    return ("bf16",) if c["fam"] == "gemm_dma" else H16
