"""fp64 references, rounding models, launch-geometry restatements and case lists of tests/test_deepresnet_ops.py (CPU)
and tests/test_deepresnet_ops_gpu.py (csrc/deepresnet_train.hip and csrc/deepresnet.hip at the C-ABI).  Plain torch; every
function runs on the device of its arguments (an fp64 matrix product on the GPU is independent of the kernels under test,
and the two large cases need it to stay within seconds).

A value the kernels compute is carried as V(ref, ea, eb): `ref` the exact (fp64) value of the formula on the bytes the
kernel read, `ea` a bound on the kernel's fp32 arithmetic error, `eb` the part of the bound that comes from an operand
that may have rounded to the other neighbour of T / a ReLU that may have flipped (see `operand` and `mask`).  The bar of a
stored element is half an ulp of T at `ref` plus ea + eb.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CODE = {"f32": 0, "bf16": 1}
ESIZE = {"f32": 4, "bf16": 2}
CO = [32, 64, 64, 64, 128, 128, 128]
CI = [1, 32, 64, 32, 64, 128, 64]
TAPS = [9, 9, 9, 1, 9, 9, 1]
EPS = 1e-5
SHARE_CAP = 0.05       # share of a checked tensor's elements whose bar may be dominated by the boundary / flip term


# ---------------------------------------------------------------------------------------------------------------------
# launch geometry (csrc/deepresnet_train.hip:1020-1094, 1168-1207, 1283-1344, 1421-1437; csrc/deepresnet.hip:199-213)
# ---------------------------------------------------------------------------------------------------------------------
MAXM, NT, MASK_ROWS, WG_GROUPS, PART_MAX, GRAPH_MAX_ROWS, LDS_CAP = 22, 512, 512, 256, 128, 1 << 17, 160 * 1024


def cdiv(a, b):
    return (a + b - 1) // b


def align256(b):
    return cdiv(b, 256) * 256


def choose_tile(dt, P):
    """-> (tile side, tiles per frame side)"""
    tsmax = 13 if dt == "bf16" else 9
    nt = cdiv(P, tsmax)
    return cdiv(P, nt), nt


def conv_image_bytes(dt, t, Fs, C):
    es = ESIZE[dt]
    if es != 2:
        return Fs * (t + 2) * (t + 2) * (C + 4) * es
    csb = (C + 16) * es
    rowb = (t + 2) * csb + (256 - (2 * csb) % 256) % 256
    spb = (((t * t * csb - (t + 2) * rowb) % 256) + 256) % 256
    return Fs * ((t + 2) * rowb + spb)


def conv_lds(dt, t, Fs, cin, cin2=0, mm=MAXM):
    return (conv_image_bytes(dt, t, Fs, cin) + (conv_image_bytes(dt, t, Fs, cin2) if cin2 else 0) + 8 * 3 * 32 * 4
            + 2 * mm * 16 * 4 + 2 * Fs * (t + 2) * (t + 2) * 4)


def wgrad_lds(dt, t, Fs, cin, cout):
    es = ESIZE[dt]
    RP = cdiv(Fs * t * t, 32) * 32
    return conv_image_bytes(dt, t, Fs, cin) + RP * (cout * es + (32 if es == 2 else 16)) + RP * 8 + 2 * Fs * (t + 2) * (t + 2) * 4


def slots_fit(t, need, mm=MAXM, cap=LDS_CAP):
    Fs = (mm * 16) // (t * t)
    while Fs >= 1 and need(Fs) > cap:
        Fs -= 1
    return Fs


def conv0_slots(t):
    return max(1, 512 // (t * t))


def train_supported(dt, P):
    if P < 1 or P > 4096:
        return False
    t, _ = choose_tile(dt, P)
    return (slots_fit(t, lambda f: conv_lds(dt, t, f, 128)) >= 1 and slots_fit(t, lambda f: wgrad_lds(dt, t, f, 128, 64)) >= 1)


def parts_cap(dt, N, P):
    _, nt = choose_tile(dt, P)
    return max(N * nt * nt, cdiv(N * P * P, MASK_ROWS)) + 8


def linear_wgrad_ws_bytes(M, N, K):
    """mivit_linear_wgrad_workspace_bytes (csrc/gemm.hip), as restated in operators_common.wgrad_ws_bytes"""
    tiles = cdiv(N, 128) * cdiv(K, 128)
    sp = max(1, min(cdiv(384, tiles), (M + 255) // 256, 512))
    chunks = 1 if M <= 256 else max(1, min(256, cdiv(M, 64 if M < 8192 else 512)))
    return align256((sp * N * K * 4 if sp > 1 else 0) + chunks * N * 4)


def ws_layout(dt, N, P, E):
    """make_ws: the 16 offsets of mivit_deepresnet_train_workspace_layout"""
    off, out = 0, {}

    def take(b):
        nonlocal off
        o = off
        off += align256(b)
        return o
    R, es = N * P * P, ESIZE[dt]
    y = [take(R * CO[i] * es) for i in range(7)]
    for i in range(7):
        take(CO[i] * CI[i] * TAPS[i] * es)
        take(CO[i] * CI[i] * TAPS[i] * es)
    fco, bco = take(7 * 4 * 128 * 4), take(7 * 3 * 128 * 4)
    pooled, dpooled = take(N * 128 * 4), take(N * 128 * 4)
    part = take(parts_cap(dt, N, P) * 3 * 128 * 4 * 2)
    take(PART_MAX * 3 * 128 * 4)
    X = [take(R * 128 * es) for _ in range(3)]
    take(WG_GROUPS // 2 * 128 * 9 * 128 * 4)
    take(linear_wgrad_ws_bytes(N, E, 128))
    return y + [fco, bco, pooled, dpooled, part] + X + [off]


def wgrad_csplit(cin, cout, taps):
    return 2 if taps * (cout // 16) * (cin // 16) // 8 > 36 else 1


def launch_plan(dt, N, P):
    """every decision the host code takes for one (dtype, N, P): what the coverage test reads"""
    t, nt = choose_tile(dt, P)
    units, R = N * nt * nt, N * P * P
    p = {"t": t, "nt": nt, "whole": nt == 1, "divides": nt > 1 and nt * t == P, "overhang": nt * t > P, "R": R, "units": units}
    convs = {}
    for name, cin in (("c32", 32), ("c64", 64), ("c128", 128)):              # forward and data-gradient passes, MM = MAXM
        Fs = slots_fit(t, lambda f: conv_lds(dt, t, f, cin))
        convs[name] = (Fs, cdiv(units, Fs))
    if dt == "bf16":                                                          # the 1x1 skip pass, half-size groups
        for name, cin in (("skip128", 128), ("skip64", 64)):
            Fh = slots_fit(t, lambda f: conv_lds(dt, t, f, cin, 0, MAXM // 2), MAXM // 2, 80 * 1024)
            convs[name] = (Fh, cdiv(units, Fh)) if Fh >= 1 else convs["c128" if cin == 128 else "c64"]
            p["half_" + name] = Fh >= 1
    F0 = conv0_slots(t)
    convs["conv0"] = (F0, cdiv(units, F0))
    p["convs"] = convs
    wg = {}
    for i in (1, 2, 3, 4, 5, 6):
        cs = wgrad_csplit(CI[i], CO[i], TAPS[i])
        Fs = slots_fit(t, lambda f: wgrad_lds(dt, t, f, CI[i], CO[i] // cs))
        ng = cdiv(units, Fs)
        wg[i] = {"csplit": cs, "F": Fs, "ngroups": ng, "G": min(ng, WG_GROUPS // cs)}
    p["wgrad"] = wg
    p["wgrad0"] = {"ngroups": convs["conv0"][1], "G": min(convs["conv0"][1], 256)}
    p["mask_parts"] = cdiv(R, MASK_ROWS)
    p["fwd_parts"] = max(b for _, b in (convs["conv0"], convs["c32"], convs["c64"], convs["c128"]))
    p["squeeze_fwd"] = p["fwd_parts"] > PART_MAX
    p["squeeze_mask"] = p["mask_parts"] > PART_MAX
    p["graph"] = R <= GRAPH_MAX_ROWS
    allF = [f for f, _ in convs.values()] + [w["F"] for w in wg.values()]
    p["F1"], p["Fmany"] = any(f == 1 for f in allF), any(f > 1 for f in allF)
    p["ragged"] = any(units % f and units > f for f in allF)
    p["dead_slots"] = N == 1 and any(f > units for f in allF)
    return p


EVAL_MAXM = 11


def eval_frames_per_block(dt, P):
    Fs = (EVAL_MAXM * 16) // (P * P)
    while Fs >= 1 and 2 * Fs * (P + 2) * (P + 2) * (128 * ESIZE[dt] + 16) + Fs * 128 * 4 > LDS_CAP:
        Fs -= 1
    return Fs


def eval_supported(dt, P):
    return P >= 3 and eval_frames_per_block(dt, P) >= 1


# ---------------------------------------------------------------------------------------------------------------------
# rounding model
# ---------------------------------------------------------------------------------------------------------------------
def rnd(x, dt):
    """fp64 -> the nearest value of T, as fp64 ("f64": the exact pipeline, used against autograd)"""
    return x if dt == "f64" else x.to(DT[dt]).double()


def rnd32(x, dt):
    return x if dt == "f64" else x.float().double()


def unit(dt):
    return 0.0 if dt == "f64" else U32


def half_ulp(ref, dt):
    """half an ulp of T at `ref`.  The rounding happens at the KERNEL's value: callers pass |ref| + the error bound, so an
    element whose reference sits just under a power of two gets the half ulp of the binade the kernel may have been in"""
    if dt != "bf16":
        return torch.zeros_like(ref)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -127))).clamp_min(-126)
    return torch.pow(2.0, e - 8)


class V:
    def __init__(self, ref, ea=None, eb=None):
        self.ref = ref
        self.ea = torch.zeros_like(ref) if ea is None else ea
        self.eb = torch.zeros_like(ref) if eb is None else eb

    @property
    def err(self):
        return self.ea + self.eb

    def flat(self, C):
        return V(self.ref.reshape(-1, C), self.ea.reshape(-1, C), self.eb.reshape(-1, C))


def fma32(dt, nops, *terms):
    """a sum of products evaluated in fp32 with `nops` roundings: each is at most one unit of the sum of magnitudes"""
    ref = sum(terms)
    return V(ref, nops * unit(dt) * sum(t.abs() for t in terms))


def operand(v, dt):
    """a value computed in fp32 and rounded to T while staged into LDS (fill_batched -> store16, deepresnet_train.hip:
    193-200): the kernel holds rnd(ref) unless ref lies within the fp32 error of a rounding boundary of T (or of zero, for
    a ReLU that `v` already went through); then it may hold the other neighbour.  -> (operand, its uncertainty)"""
    a = rnd(v.ref, dt)
    d = rnd(v.ref + v.err, dt) - rnd(v.ref - v.err, dt)
    return a, d


def relu(v):
    return V(v.ref.clamp_min(0), v.ea, v.eb)            # 1-Lipschitz


def mask(v, act):
    """v * [act > 0] with act computed in fp32: the mask may differ only where |act| is within its fp32 error of zero"""
    on = (act.ref > 0).to(v.ref.dtype)
    flip = (act.ref.abs() <= act.err).to(v.ref.dtype)
    return V(v.ref * on, v.ea * torch.maximum(on, flip), v.eb * torch.maximum(on, flip) + v.ref.abs() * flip)


def conv64(A, Wp):
    """A [N,P,P,Ci], Wp [Co, taps, Ci] (tap = 3 ky + kx, zero padding) -> [N,P,P,Co]"""
    N, P, _, Ci = A.shape
    Co, taps, _ = Wp.shape
    if taps == 1:
        return (A.reshape(-1, Ci) @ Wp[:, 0, :].t()).reshape(N, P, P, Co)
    Ap = F.pad(A, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(N * P * P, Co, dtype=A.dtype, device=A.device)
    for t in range(9):
        out += Ap[:, t // 3:t // 3 + P, t % 3:t % 3 + P, :].reshape(-1, Ci) @ Wp[:, t, :].t()
    return out.reshape(N, P, P, Co)


def _bar32(fn, a, b, *more):
    """a bar term (non-negative operands) needs no fp64: fp32 products, widened by more than their own rounding"""
    if not bool((a != 0).any()):
        return torch.zeros((), dtype=torch.float64, device=a.device)
    return fn(a.float(), b.float(), *more).double() * (1 + 1e-4)


def conv_v(dt, a, da, Wp, kred, extra=None):
    """fp32-accumulated convolution of a staged operand (a, uncertainty da); `extra`: a V the accumulators start from"""
    ref = conv64(a, Wp)
    ea = (kred + 1) * unit(dt) * _bar32(conv64, a.abs(), Wp.abs())
    eb = _bar32(conv64, da, Wp.abs())
    if extra is not None:
        ref, ea, eb = ref + extra.ref, ea + extra.ea + unit(dt) * extra.ref.abs(), eb + extra.eb
    return V(ref, ea, eb) if dt == "bf16" else V(ref, ea + eb)


def wgrad64(D, A, taps):
    """D [N,P,P,Co], A [N,P,P,Ci] -> dW [Co, Ci, taps] = sum_r D[r] A[pixel(r) + tap]"""
    N, P, _, Ci = A.shape
    Co = D.shape[-1]
    Dm = D.reshape(-1, Co).t()
    if taps == 1:
        return (Dm @ A.reshape(-1, Ci))[:, :, None]
    Ap = F.pad(A, (0, 0, 1, 1, 1, 1))
    return torch.stack([Dm @ Ap[:, t // 3:t // 3 + P, t % 3:t % 3 + P, :].reshape(-1, Ci) for t in range(9)], dim=2)


def wgrad_v(dt, d, dd, a, da, taps):
    R = d.shape[0] * d.shape[1] * d.shape[2]
    ref = wgrad64(d, a, taps)
    ea = (R + WG_GROUPS + 1) * unit(dt) * _bar32(wgrad64, d.abs(), a.abs(), taps)
    eb = _bar32(wgrad64, dd, a.abs() + da, taps) + _bar32(wgrad64, d.abs(), da, taps)
    return V(ref, ea, eb) if dt == "bf16" else V(ref, ea + eb)


def pack_fwd(W, dt):
    """Conv2d weight [co, ci, kh, kw] -> rnd_T, [co][tap][ci] (drn_pack_kernel)"""
    co, ci = W.shape[:2]
    return rnd(W.double(), dt).reshape(co, ci, -1).permute(0, 2, 1).contiguous()


def pack_dgrad(W, dt):
    """... -> [ci][taps-1-tap][co]: the data gradient is a convolution of dy with the flipped taps"""
    co, ci = W.shape[:2]
    return rnd(W.double(), dt).reshape(co, ci, -1).flip(2).permute(1, 2, 0).contiguous()


# summation depth of the fp32 partial sums: no partial is the end of a longer chain of additions than this
#   conv epilogue (deepresnet_train.hip:423-454): MT <= 22 row tiles per lane, 4 shuffle levels, MQ <= 4 waves, the product
#   conv0 (:565-581) and the mask kernel (:800-830): <= 32 rows per thread, then 16 (32) partials in sequence
# and squeeze_parts rounds the fp64 sum of several partials to fp32 once more (counted in the depth).  The number of
# partials does not enter: drn_bn_finalize_kernel, drn_part_reduce_kernel and drn_sync_reduce_kernel add them in fp64, where
# n_partials * 2^-53 is nothing beside one fp32 rounding of a single partial.
D_CONV, D_SEQ = 32, 68


def sums(dt, depth, v, *weights):
    """per-channel sums of v * w over the rows (w = 1 when omitted): -> V [C]"""
    out = []
    for w in weights or (None,):
        r = v.ref if w is None else v.ref * w
        e = v.err if w is None else v.err * w.abs()
        out.append(V(r.sum(0), (depth + (w is not None)) * unit(dt) * r.abs().sum(0) + e.sum(0)))
    return out if len(out) > 1 else out[0]


def bn_table(dt, s, q, n, gamma, beta, eps):
    """drn_bn_finalize_kernel (:669-695).  s, q: V of the sum and the sum of squares.  -> V [4, C] mean|rstd|scale|shift,
    and V of the batch mean / unbiased variance the running statistics take.  The variance is E[x^2] - mean^2: its bar is
    the error of the two sums, which cancels against var, not against E[x^2]."""
    u = unit(dt)
    mean, dmean = s.ref / n, s.err / n
    ex2 = q.ref / n
    var = (ex2 - mean * mean).clamp_min(0)
    dvar = q.err / n + 2 * mean.abs() * dmean + dmean * dmean
    rstd = 1 / torch.sqrt(var + eps)
    lo, hi = 1 / torch.sqrt(var + dvar + eps), 1 / torch.sqrt((var - dvar).clamp_min(0) + eps)
    drstd = torch.maximum(hi - rstd, rstd - lo) + u * rstd
    scale = gamma * rstd
    dscale = gamma.abs() * drstd + u * scale.abs()
    shift = beta - mean * scale
    dshift = scale.abs() * (dmean + u * mean.abs()) + mean.abs() * dscale + 2 * u * (beta.abs() + (mean * scale).abs())
    tab = V(torch.stack([mean, rstd, scale, shift]), torch.stack([dmean + u * mean.abs(), drstd, dscale, dshift]))
    ub = n / (n - 1) if n > 1 else 1.0
    return tab, V(mean, dmean + u * mean.abs()), V(var * ub, dvar * ub + u * var * ub)


def running_update(dt, r0, batch, m):
    ref = (1 - m) * r0 + m * batch.ref
    return V(ref, m * batch.err + 3 * unit(dt) * (((1 - m) * r0).abs() + (m * batch.ref).abs()))


def running_table(dt, gamma, beta, rm, rv, eps):
    """drn_bn_running_kernel (:698-704), all in fp32"""
    u = unit(dt)
    rstd = 1 / torch.sqrt(rv + eps)
    drstd = 4 * u * rstd
    scale = gamma * rstd
    dscale = gamma.abs() * drstd + u * scale.abs()
    shift = beta - rm * scale
    dshift = rm.abs() * dscale + 2 * u * (beta.abs() + (rm * scale).abs())
    return V(torch.stack([rm, rstd, scale, shift]), torch.stack([torch.zeros_like(rm), drstd, dscale, dshift]))


def bn_bwd_table(dt, s, q, n, gamma, ftab):
    """drn_bn_bwd_finalize_kernel (:836-864) on the kernel's own forward table.  -> (V [3, C] k|c0|c1, dgamma, dbeta).
    dgamma = rstd * (sum g y - mean * sum g): un-centred, so its bar is |mean| * the error of sum g plus that of sum g y"""
    u = unit(dt)
    mean, rstd = ftab[0], ftab[1]
    dg = rstd * (q.ref - mean * s.ref)
    ddg = rstd * (q.err + mean.abs() * s.err)
    k = gamma * rstd
    c1 = -k * rstd * dg / n
    dc1 = (k * rstd / n).abs() * ddg
    c0 = -k * s.ref / n - c1 * mean
    dc0 = k.abs() * s.err / n + mean.abs() * dc1
    tab = V(torch.stack([k, c0, c1]), torch.stack([u * k.abs(), dc0 + u * c0.abs(), dc1 + u * c1.abs()]))
    return tab, V(dg, ddg + u * dg.abs()), V(s.ref, s.err + u * s.ref.abs())


# ---------------------------------------------------------------------------------------------------------------------
# the walk: every stage's reference from the bytes that stage read
# ---------------------------------------------------------------------------------------------------------------------
class Walk:
    """`got`: name -> what the kernel left (fp64 copies).  A name in `got` is compared with its reference and handed on
    as the operand of the next stage, so errors do not compound.  A name that is absent is simulated (rnd(ref)): with
    got = {} the walk is the reference model alone (CPU tests); with `regen` = names the run could not keep (the
    single-call backward overwrites g2 and g21) the regenerated buffer carries its own uncertainty on."""

    def __init__(self, dt, got=None, regen=()):
        self.dt, self.got, self.regen, self.rec, self.sim, self.ref = dt, got or {}, set(regen), {}, {}, {}

    def out(self, name, v, kind="T"):
        """kind "T": stored in the compute type; "f32": an fp32 value.  -> (value the next stage reads, its uncertainty)"""
        dt = self.dt
        if kind == "T":
            bar_a = half_ulp(v.ref.abs() + v.err, dt) + v.ea + (unit(dt) * v.ref.abs() if dt == "f32" else 0)
            val = rnd(v.ref, dt)
        else:
            bar_a = v.ea + unit(dt) * v.ref.abs()
            val = rnd32(v.ref, dt)
        if name in self.got:
            g = self.got[name].reshape(v.ref.shape)
            if name[:3] in ("fco", "dga"):
                self.ref[name] = v.ref
            err = (g - v.ref).abs()
            bar = bar_a + v.eb
            ratio = torch.where(err > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
            i = int(ratio.argmax())
            self.rec[name] = {"ratio": float(ratio.flatten()[i]), "err": float(err.flatten()[i]), "bar": float(bar.flatten()[i]),
                              "index": i, "share": float((v.eb > bar_a).double().mean()), "finite": bool(torch.isfinite(g).all())}
            return g, torch.zeros_like(g)
        self.sim[name] = val
        self.rec.setdefault(name, {"ratio": 0.0, "err": 0.0, "bar": 0.0, "index": -1, "finite": True,
                                   "share": float((v.eb > bar_a).double().mean())})
        if name in self.regen:
            return val, (rnd(v.ref + v.err, dt) - rnd(v.ref - v.err, dt)) if kind == "T" else 2 * v.err
        return val, torch.zeros_like(val)


def _nhwc(t, N, P):
    return t.reshape(N, P, P, -1)


def act1_pre(dt, y, tab):
    return fma32(dt, 2, tab[2] * y, tab[3].expand_as(y))


def act2_pre(dt, y, tab, y2, tab2):
    return fma32(dt, 5, tab[2] * y, tab[3].expand_as(y), tab2[2] * y2, tab2[3].expand_as(y))


def dy_v(dt, g, dg, y, bt):
    """k*g + c0 + c1*y (PRO_DY); dg: uncertainty of a regenerated g"""
    v = fma32(dt, 4, bt[0] * g, bt[1].expand_as(g), bt[2] * y)
    return V(v.ref, v.ea, bt[0].abs() * dg)


def walk_forward(w, prm, x, N, P, E, eps=EPS, momentum=0.1, running=True, infer=False):
    """prm: {"W": [7 Conv2d weights], "gamma", "beta", "rm", "rv": [7 vectors], "fcw", "fcb"}, fp64 copies of the fp32
    parameters (running statistics BEFORE the call).  x [N,P,P].  Fills w.rec; -> dict of what the backward reads."""
    dt, n = w.dt, N * P * P
    y, tab = [None] * 7, [None] * 7

    def finish(i, v, depth):
        vf = v.flat(CO[i])
        y[i], _ = w.out(f"y{i}", vf)
        if infer:
            t = running_table(dt, prm["gamma"][i], prm["beta"][i], prm["rm"][i], prm["rv"][i], eps)
        else:
            s = sums(dt, depth, vf)
            q = V((vf.ref * vf.ref).sum(0), (depth + 1) * unit(dt) * (vf.ref * vf.ref).sum(0) + ((2 * vf.ref.abs() + vf.err) * vf.err).sum(0))
            t, bm, bv = bn_table(dt, s, q, n, prm["gamma"][i], prm["beta"][i], eps)
            if running:
                w.out(f"rm{i}", running_update(dt, prm["rm"][i], bm, momentum), "f32")
                w.out(f"rv{i}", running_update(dt, prm["rv"][i], bv, momentum), "f32")
        tab[i], _ = w.out(f"fco{i}", t, "f32")

    # conv0: VALU, fp32 frames and weights (:547-582)
    w0 = prm["W"][0].reshape(32, 1, 9).permute(0, 2, 1)
    xi = x.reshape(N, P, P, 1)
    finish(0, V(conv64(xi, w0), 10 * unit(dt) * conv64(xi.abs(), w0.abs())), D_SEQ)
    a0, da0 = operand(relu(act1_pre(dt, _nhwc(y[0], N, P), tab[0])), dt)
    finish(1, conv_v(dt, a0, da0, pack_fwd(prm["W"][1], dt), 9 * 32), D_CONV)
    finish(3, conv_v(dt, a0, da0, pack_fwd(prm["W"][3], dt), 32), D_CONV)
    a11, da11 = operand(relu(act1_pre(dt, _nhwc(y[1], N, P), tab[1])), dt)
    finish(2, conv_v(dt, a11, da11, pack_fwd(prm["W"][2], dt), 9 * 64), D_CONV)
    o1, do1 = operand(relu(act2_pre(dt, _nhwc(y[2], N, P), tab[2], _nhwc(y[3], N, P), tab[3])), dt)
    finish(4, conv_v(dt, o1, do1, pack_fwd(prm["W"][4], dt), 9 * 64), D_CONV)
    finish(6, conv_v(dt, o1, do1, pack_fwd(prm["W"][6], dt), 64), D_CONV)
    a21, da21 = operand(relu(act1_pre(dt, _nhwc(y[4], N, P), tab[4])), dt)
    finish(5, conv_v(dt, a21, da21, pack_fwd(prm["W"][5], dt), 9 * 128), D_CONV)
    # pooling (:734-770): V = 16 / sizeof(T) pixel sets, each a chain of ceil(PP / V) additions, then V more and the division
    o2 = relu(act2_pre(dt, y[5], tab[5], y[6], tab[6]))
    nps = 8 if dt == "bf16" else 4
    depth = cdiv(P * P, nps) + nps + 1
    pr = o2.ref.reshape(N, P * P, 128)
    pooled, _ = w.out("pooled", V(pr.mean(1), o2.err.reshape(N, P * P, 128).mean(1) + depth * unit(dt) * pr.abs().mean(1)), "f32")
    tok = pooled @ prm["fcw"].t() + prm["fcb"]
    w.out("tokens", V(tok, 2 * 129 * unit(dt) * (pooled.abs() @ prm["fcw"].abs().t() + prm["fcb"].abs())), "f32")
    return {"y": y, "tab": tab, "pooled": pooled, "ops": {"a0": (a0, da0), "a11": (a11, da11), "o1": (o1, do1), "a21": (a21, da21)}}


def walk_backward(w, prm, x, dtok, fw, N, P, E):
    """fw: what walk_forward returned for the same workspace.  dtok [N,E]."""
    dt, n, u = w.dt, N * P * P, unit(w.dt)
    y, tab, ops = fw["y"], fw["tab"], fw["ops"]
    Y = [_nhwc(t, N, P) for t in y]
    # stage 0: the Linear, then the pooling gradient masked by the output ReLU (:1359-1373, 782-831)
    dp, _ = w.out("dpooled", V(dtok @ prm["fcw"], (E + 1) * u * (dtok.abs() @ prm["fcw"].abs())), "f32")
    w.out("dfcw", V(dtok.t() @ fw["pooled"], (N + 9) * u * (dtok.abs().t() @ fw["pooled"].abs())), "f32")
    w.out("dfcb", V(dtok.sum(0), (N + 9) * u * dtok.abs().sum(0)), "f32")
    up = (dp / (P * P))[:, None, None, :].expand(N, P, P, 128)
    g2v = mask(V(up, 2 * u * up.abs()), act2_pre(dt, Y[5], tab[5], Y[6], tab[6])).flat(128)
    g2, dg2 = w.out("g2", g2v)
    s, qa, qb = sums(dt, D_SEQ, g2v, None, y[5], y[6])
    bt, bdt = [None] * 7, {}

    def table(i, s_, q_):
        t, dgam, dbet = bn_bwd_table(dt, s_, q_, n, prm["gamma"][i], tab[i])
        bt[i], _ = w.out(f"bco{i}", t, "f32")
        w.out(f"dgamma{i}", dgam, "f32")
        w.out(f"dbeta{i}", dbet, "f32")

    def wg(i, d, a):
        w.out(f"dW{i}", wgrad_v(dt, d[0], d[1], a[0], a[1], TAPS[i]).flat(1), "f32")

    def stage_dy(g, dg, yi, i):
        return operand(dy_v(dt, _nhwc(g, N, P), _nhwc(dg, N, P), Y[yi], bt[i]), dt)

    # stage 1: BatchNorm 5 / 6, their weight gradients, d a21 masked -> g21 (:1374-1384)
    table(5, s, qa)
    table(6, s, qb)
    dy22, dy2s = stage_dy(g2, dg2, 5, 5), stage_dy(g2, dg2, 6, 6)
    wg(5, dy22, ops["a21"])
    wg(6, dy2s, ops["o1"])
    g21v = mask(conv_v(dt, dy22[0], dy22[1], pack_dgrad(prm["W"][5], dt), 9 * 128), act1_pre(dt, Y[4], tab[4])).flat(128)
    g21, dg21 = w.out("g21", g21v)
    s, qa = sums(dt, D_CONV, g21v, None, y[4])
    # stage 2: BatchNorm 4; d o1 = 3x3 pass (stored in T), + the skip's 1x1 pass, masked -> g1 (:1385-1398)
    table(4, s, qa)
    dy21 = stage_dy(g21, dg21, 4, 4)
    wg(4, dy21, ops["o1"])
    tv = conv_v(dt, dy21[0], dy21[1], pack_dgrad(prm["W"][4], dt), 9 * 128)
    tvs = V(tv.ref, tv.ea + half_ulp(tv.ref.abs() + tv.err, dt), tv.eb)        # the 3x3 pass leaves rnd_T(t); the skip pass reads it back
    g1v = mask(conv_v(dt, dy2s[0], dy2s[1], pack_dgrad(prm["W"][6], dt), 128, extra=tvs),
               act2_pre(dt, Y[2], tab[2], Y[3], tab[3])).flat(64)
    g1, dg1 = w.out("g1", g1v)
    s, qa, qb = sums(dt, D_CONV, g1v, None, y[2], y[3])
    # stage 3: BatchNorm 2 / 3; d a11 masked -> g11 (:1399-1408)
    table(2, s, qa)
    table(3, s, qb)
    dy12, dy1s = stage_dy(g1, dg1, 2, 2), stage_dy(g1, dg1, 3, 3)
    wg(2, dy12, ops["a11"])
    wg(3, dy1s, ops["a0"])
    g11v = mask(conv_v(dt, dy12[0], dy12[1], pack_dgrad(prm["W"][2], dt), 9 * 64), act1_pre(dt, Y[1], tab[1])).flat(64)
    g11, dg11 = w.out("g11", g11v)
    s, qa = sums(dt, D_CONV, g11v, None, y[1])
    # stage 4: BatchNorm 1; d a0 = 3x3 pass + skip pass, masked -> g0 (:1409-1420)
    table(1, s, qa)
    dy11 = stage_dy(g11, dg11, 1, 1)
    wg(1, dy11, ops["a0"])
    tv = conv_v(dt, dy11[0], dy11[1], pack_dgrad(prm["W"][1], dt), 9 * 64)
    tvs = V(tv.ref, tv.ea + half_ulp(tv.ref.abs() + tv.err, dt), tv.eb)        # the 3x3 pass leaves rnd_T(t); the skip pass reads it back
    g0v = mask(conv_v(dt, dy1s[0], dy1s[1], pack_dgrad(prm["W"][3], dt), 64, extra=tvs), act1_pre(dt, Y[0], tab[0])).flat(32)
    g0, dg0 = w.out("g0", g0v)
    s, qa = sums(dt, D_CONV, g0v, None, y[0])
    # stage 5: BatchNorm 0 and the first convolution's weight gradient: dy0 stays in fp32 registers, the frames are fp32
    table(0, s, qa)
    d0 = dy_v(dt, _nhwc(g0, N, P), _nhwc(dg0, N, P), Y[0], bt[0])
    xi = x.reshape(N, P, P, 1)
    w.out("dW0", V(wgrad64(d0.ref, xi, 9), (n + 257) * u * wgrad64(d0.ref.abs(), xi.abs(), 9) + wgrad64(d0.err, xi.abs(), 9)).flat(1), "f32")


# ---------------------------------------------------------------------------------------------------------------------
# fused inference kernel (csrc/deepresnet.hip): BatchNorm folded in fp64 by the test, weights rounded to T by the test
# ---------------------------------------------------------------------------------------------------------------------
def fold64(prm, dt, eps=EPS):
    """-> pack of fp64 tensors: w0 [32,9], b0, w11 .. w2s [co, taps*ci] (values of T), b11, b12, b21, b22, wfc, bfc"""
    def fold(i, t):
        a = prm["gamma"][i] / torch.sqrt(prm["rv"][i] + eps)
        co, ci = prm["W"][i].shape[:2]
        wf = (prm["W"][i].double() * a.view(-1, 1, 1, 1)).reshape(co, ci, -1).permute(0, 2, 1).reshape(co, -1)
        return rnd(wf, t), rnd32(prm["beta"][i] - prm["rm"][i] * a, t)
    pk = {}
    f32 = "f64" if dt == "f64" else "f32"
    pk["w0"], pk["b0"] = fold(0, f32)
    (pk["w11"], pk["b11"]), (pk["w12"], b12), (pk["w1s"], b1s) = fold(1, dt), fold(2, dt), fold(3, dt)
    (pk["w21"], pk["b21"]), (pk["w22"], b22), (pk["w2s"], b2s) = fold(4, dt), fold(5, dt), fold(6, dt)
    pk["b12"], pk["b22"] = rnd32(b12 + b1s, f32), rnd32(b22 + b2s, f32)
    pk["wfc"], pk["bfc"] = prm["fcw"], prm["fcb"]
    return pk


def eval_tokens(dt, pk, x, N, P):
    """-> V of the tokens.  Nothing between the frames and the tokens is observable, so the uncertainty of every staged
    activation (rounded to T in LDS, deepresnet.hip:96, :129) is carried through the layers."""
    u = unit(dt)

    def layer(a, da, wname, cin, taps, bias, extra=None):
        Wp = pk[wname].reshape(-1, taps, cin)
        v = conv_v(dt, a, da, Wp, taps * cin, extra=extra)
        return v if bias is None else V(v.ref + bias, v.ea + u * (v.ref.abs() + bias.abs()), v.eb)
    xi = x.reshape(N, P, P, 1)
    w0 = pk["w0"].reshape(32, 9, 1)
    c0 = conv64(xi, w0) + pk["b0"]
    a0, da0 = operand(relu(V(c0, 10 * u * (conv64(xi.abs(), w0.abs()) + pk["b0"].abs()))), dt)
    t1, dt1 = operand(relu(layer(a0, da0, "w11", 32, 9, pk["b11"])), dt)
    o1, do1 = operand(relu(layer(a0, da0, "w1s", 32, 1, pk["b12"], extra=layer(t1, dt1, "w12", 64, 9, None))), dt)
    t2, dt2 = operand(relu(layer(o1, do1, "w21", 64, 9, pk["b21"])), dt)
    o2 = relu(layer(o1, do1, "w2s", 64, 1, pk["b22"], extra=layer(t2, dt2, "w22", 128, 9, None)))
    depth = P * P + 3
    pr = o2.ref.reshape(N, P * P, 128)
    pool = V(pr.mean(1), o2.ea.reshape(N, P * P, 128).mean(1) + depth * u * pr.abs().mean(1), o2.eb.reshape(N, P * P, 128).mean(1))
    aw = pk["wfc"].abs().t()
    tok = pool.ref @ pk["wfc"].t() + pk["bfc"]
    return V(tok, pool.ea @ aw + 130 * u * (pool.ref.abs() @ aw + pk["bfc"].abs()), pool.eb @ aw)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and cases
# ---------------------------------------------------------------------------------------------------------------------
def make_params(seed, E, adversarial=False):
    """fp32 parameters in the reference's layouts, randomised affine and running statistics"""
    g = torch.Generator().manual_seed(seed)
    p = {"W": [], "gamma": [], "beta": [], "rm": [], "rv": []}
    for i in range(7):
        fan = CI[i] * TAPS[i]
        k = 3 if TAPS[i] == 9 else 1
        p["W"].append(torch.randn(CO[i], CI[i], k, k, generator=g) * (2.0 / fan) ** 0.5)
        p["gamma"].append(0.7 + 0.6 * torch.rand(CO[i], generator=g))
        p["beta"].append(0.1 * torch.randn(CO[i], generator=g))
        p["rm"].append(0.2 * torch.randn(CO[i], generator=g))
        p["rv"].append(0.5 + torch.rand(CO[i], generator=g))
    p["fcw"] = torch.randn(E, 128, generator=g) / 128 ** 0.5
    p["fcb"] = 0.1 * torch.randn(E, generator=g)
    if adversarial:
        # channel 3 of every MFMA convolution: zero weights -> variance exactly 0, rstd = 1 / sqrt(eps)
        for i in range(1, 7):
            p["W"][i][3] = 0
        # channel 5 of the first convolution: the centre tap alone, on frames of a DC level 1 with a ripple of 1e-3
        # (make_frames "dc"): its variance is 1e-6 of its squared mean
        p["W"][0][5] = 0
        p["W"][0][5, 0, 1, 1] = 1.0
    return p


def make_frames(kind, N, P, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "rand":
        return torch.rand(N, P, P, generator=g) * 1.5 - 0.25
    if kind == "counts":
        yy, xx = torch.meshgrid(torch.arange(P, dtype=torch.float32), torch.arange(P, dtype=torch.float32), indexing="ij")
        cen = (P - 1) / 2 + 1.5 * torch.randn(N, 2, generator=g)
        spot = torch.exp(-((yy - cen[:, 0, None, None]) ** 2 + (xx - cen[:, 1, None, None]) ** 2) / (2 * 1.1 ** 2))
        return 5000.0 + 70.0 * torch.randn(N, P, P, generator=g) + 5000.0 * spot
    if kind == "dc":
        return 1.0 + 1e-3 * torch.randn(N, P, P, generator=g)
    raise ValueError(kind)


def to64(p, device="cpu"):
    return {k: ([t.double().to(device) for t in v] if isinstance(v, list) else v.double().to(device)) for k, v in p.items()}


def _c(**kw):
    return kw


# the smallest shapes that reach each branch; `dts` = the dtypes whose geometry the case is chosen for
CASES = [
    _c(id="whole-9x9-ragged", N=5, P=9, E=64, x="rand"),
    _c(id="P1-N300-null-running", N=300, P=1, E=1, x="rand", running=False, dw_cap=0.15),
    _c(id="P2-N75", N=75, P=2, E=16, x="rand", momentum=1.0, dw_cap=0.10),
    _c(id="N1-P5-dead-slots", N=1, P=5, E=16, x="rand"),
    _c(id="divides-10", N=3, P=10, E=16, x="rand", dts=("f32",)),
    _c(id="overhang-13", N=2, P=13, E=130, x="rand", dts=("f32",)),
    _c(id="three-tiles-19", N=1, P=19, E=16, x="rand", dts=("f32",)),
    _c(id="whole-13", N=3, P=13, E=130, x="rand", dts=("bf16",)),
    _c(id="divides-14", N=3, P=14, E=16, x="rand", dts=("bf16",)),
    _c(id="three-tiles-overhang-29", N=1, P=29, E=16, x="rand", dts=("bf16",)),
    _c(id="camera-counts", N=6, P=9, E=64, x="counts", momentum=1.0),
    _c(id="adversarial-statistics", N=12, P=7, E=16, x="dc", adversarial=True, dw_cap=0.15),
    _c(id="squeeze-820", N=820, P=9, E=16, x="rand", large=True),
    _c(id="no-graph-1620", N=1620, P=9, E=16, x="rand", large=True),
]
SUBSET = ("whole-9x9-ragged", "N1-P5-dead-slots", "camera-counts")      # what each environment switch is run on


def case_dts(c):
    return c.get("dts", ("f32", "bf16"))


def case_inputs(c):
    prm = make_params(1000 + c["N"] * 7 + c["P"], c["E"], c.get("adversarial", False))
    x = make_frames(c["x"], c["N"], c["P"], 77 + c["P"])
    dtok = torch.randn(c["N"], c["E"], generator=torch.Generator().manual_seed(5 + c["N"]))
    return prm, x, dtok


# what the share cap is asserted on: tensors whose operands are rounded to T inside the kernel
SHARE_NAMES = tuple(f"y{i}" for i in range(1, 7)) + ("g21", "g1", "g11", "g0") + tuple(f"dW{i}" for i in range(1, 7))


def share_cap(c, name=""):
    """SHARE_CAP for every tensor of every case, except the weight gradients of the three cases that carry `dw_cap`.
    A weight gradient is an fp32 output: its bar has no final-rounding term, so ONE operand among the 2 R products of an
    element that may have rounded to the other neighbour of T outweighs the accumulation term (a root-sum-square of the
    flips would not change that: one flip is its own root-sum-square).  With frame sides 1 and 2 a 3x3 convolution is
    mostly zero padding, reductions are short and dy = k g + c0 + c1 y is evaluated un-centred, so its fp32 error is a
    larger part of an ulp; in the adversarial case the whole low-variance input channel of dW1 is of that kind.  Shares
    from the reference alone (CPU, bf16): P = 1 0.135 (dW6), P = 2 0.066 (dW4), adversarial 0.111 (dW1); every other case
    at most 0.036, the two large ones 0.002."""
    return c.get("dw_cap", SHARE_CAP) if name.startswith("dW") else SHARE_CAP


def eval_cases():
    """fused inference kernel: every supported frame side of both dtypes x (1, 2 F, 2 F + 1) frames, F = frames per block"""
    return [(dt, P, N) for dt in ("f32", "bf16") for P in range(1, 64) if eval_supported(dt, P)
            for N in sorted({1, 2 * eval_frames_per_block(dt, P), 2 * eval_frames_per_block(dt, P) + 1})]


def worst(rec, names=None):
    items = [(k, r) for k, r in rec.items() if (names is None or k in names) and r["index"] >= 0]
    return max(items, key=lambda kr: kr[1]["ratio"]) if items else (None, None)
