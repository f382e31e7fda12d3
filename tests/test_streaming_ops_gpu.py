"""The streaming GEMM family at the operator level of the C-ABI -- mivit_rowstream_*, mivit_wavestream_*, mivit_gemm_dma_*,
mivit_wgrad_bf16, mivit_wgrad_small, mivit_embed_small_*, mivit_embed_fwd_bf16 / _wgrad_bf16 and their _f16 builds -- with what
the engine passes and the older tests never did: real leading dimensions, pointers offset into their allocation, y_preact and
padding columns, every epilogue, both element types, every selectable variant (mivit_gemm_dma_set_variant 0..11, 19..37,
mivit_embed_set_variant, mivit_wgrad_bf16_set_config 21 / 22 / 31 / 32) and the row-stream kernels behind the default wave-stream
picks (mivit_rowstream_set_wavestream 0 / 1 / 2).  Rounding model, references, restated dispatch and the case tables:
tests/streaming_common.py; tests/test_streaming_ops.py asserts on the CPU that the tables reach every instantiation.

EXACT cases: small-integer operands, torch.equal against the integer reference.  ACCURACY cases: random operands |x| ~ 1
against the UNROUNDED fp64 reference, element by element, with the bar of tests/test_operators_gpu.py: half an ulp of the
element type at the element + K_red * 2^-24 * (|A| @ |B|) on the staged values (x 2 where bias / activation / residual follow;
K_red = contraction length, + the slab count for weight gradients); GELU, gelu' and the fused LayerNorm add 4 x the worst error
of the fp32 CPU restatement on the test's own inputs (never below 2^-24) times the row's scale.  The fused LayerNorm is judged
on the z the kernel stored.  No bar is scaled.
Memory: inputs strided (ld = width + 8 / + 24), 16 bytes into their allocation, NaN in all padding; outputs with padding columns,
a sentinel everywhere outside the result and a guard row before and after, checked bitwise after each call (`Out.read`);
workspaces exactly the size the query returns, with a guard behind them.

Worst error / bar seen on the MI355X (the `_report_worst` fixture prints them), bf16 / fp16: rowstream_fwd 1.000 / 0.999 (both
the fused LayerNorm's ln_out), rowstream_dgrad 0.989 / 0.943, wavestream_fwd 1.000 / 0.999 (ln_out), wavestream_dgrad 0.995 /
0.975, gemm_dma_fwd 0.982 (bf16 only), gemm_dma_dgrad 0.978, embed_small_fwd 0.994 / 0.971, embed_large_fwd 0.976 / 0.879,
wgrad_bf16 0.002 / 0.002, wgrad_small 0.001 / 0.001, embed_small_wgrad 0.001 / 0.001, embed_large_wgrad 0.004 / 0.004.  As in
the operator suite the 16-bit bars are almost all final rounding (a ratio of 1.000: the worst element sat next to a rounding
boundary), and the weight gradients' bound grows with the reduction length and is far from attained.  No case needed a wider
bar and no kernel fault was found.  All 534 GPU cases take 5.6 s.
"""
import ctypes

import pytest
import torch

import operators_common as oc
import streaming_common as sc
from gpu_buffers import SENT, Out, inp
from operators_common import DT, ESIZE

gpu = pytest.mark.gpu
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (ep, dt), (ratio, e, b, what) in sorted(_WORST.items()):
        print(f"[streaming] {ep:22s} {dt:4s} worst {e:.3e} = {ratio:.3f} of its bar {b:.3e}  ({what})")


def _check(ep, dt, what, got, ref, bar):
    assert bool(torch.isfinite(got.double()).all()), f"{ep} {dt} {what}: non-finite output"
    ratio, e, b, row = oc.row_ratio(got, ref, bar)
    print(f"[streaming] {ep} {dt} {what}: row {row} error {e:.3e} bar {b:.3e} ratio {ratio:.3f}")
    if ratio >= _WORST.get((ep, dt), (-1,))[0]:
        _WORST[(ep, dt)] = (ratio, e, b, what)
    assert ratio <= 1.0, f"{ep} {dt} {what}: error is {ratio:.3f} of its bar"


def _N():
    from moleculardiffusion_mivit_amd import _native as N
    return N


def _fn(name, dt):
    return getattr(_N().lib, name + ("_f16" if dt == "f16" else ""))


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _params(cases):
    return [pytest.param(dt, c, id=f"{dt}-{c['id']}") for c in cases for dt in sc.case_dts(c)]


@pytest.fixture
def switches():
    """set(setter name, dt, value): every switch set through it gets its previous value back at teardown"""
    undo = []

    def set_(name, dt, value):
        f = _fn(name, dt)
        undo.append((f, f(value)))
    yield set_
    for f, old in reversed(undo):
        f(old)


def _apply_switches(switches, c, dt):
    if c["fam"] == "rowstream":
        switches("mivit_rowstream_set_wavestream", dt, c.get("ws_mode", 2))
        switches("mivit_rowstream_set_wavestream_mask", dt, 7)
    if c["fam"] == "gemm_dma":
        switches("mivit_gemm_dma_set_variant", "bf16", c.get("variant", 0))
    if c["fam"] == "wgrad_bf16":
        switches("mivit_wgrad_bf16_set_config", dt, c.get("cfg", 0))
    if c["fam"] == "embed_large":
        switches("mivit_embed_set_variant", dt, c.get("variant", 0))


# ---------------------------------------------------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------------------------------------------------
def _w(W, dt):
    return W.to(DT[dt]).contiguous().cuda()


def run_fwd(c, dt, o):
    """-> dict(y, pre, ln, mean, rstd)"""
    N_ = _N()
    M, N, K = c["M"], c["N"], c["K"]
    pad, off = c["pad"], c["off"]
    ldx, ldy, ldr = K + pad, N + pad, N + 32 - pad
    xb, xp = inp(o["x"], dt, ldx, off)
    Wg = _w(o["W"], dt)
    bg = o["bias"].cuda() if o.get("bias") is not None else None
    rb, rp = inp(o["resid"], dt, ldr, off) if o.get("resid") is not None else (None, None)
    y = Out(dt, M, N, ldy, off)
    pre = Out(dt, M, N, ldy, off) if c.get("pre") else None
    args = [xp, ldx, _p(Wg), _p(bg), M, N, K, c.get("act", 0), rp, ldr if rp else 0, y.ptr, ldy, pre.ptr if pre else None]
    ln = mean = rstd = None
    if c["fam"] != "gemm_dma":
        if c.get("ln"):
            ln, mean, rstd = Out(dt, M, N, N), Out("f32", 1, M, M), Out("f32", 1, M, M)
            gg, eg = o["gamma"].cuda(), o["beta"].cuda()
            args += [_p(gg), _p(eg), ln.ptr, mean.ptr, rstd.ptr]
        else:
            args += [None] * 5
    name = f"mivit_{c['fam']}_fwd"
    N_.check(_fn(name, dt if c["fam"] != "gemm_dma" else "bf16")(*args, _st()), name)
    torch.cuda.synchronize()
    return dict(y=y.read(), pre=pre.read() if pre else None, ln=ln.read() if ln else None,
                mean=mean.read()[0] if mean else None, rstd=rstd.read()[0] if rstd else None)


def run_dgrad(c, dt, o):
    N_ = _N()
    M, N, K = c["M"], c["N"], c["K"]
    pad, off = c["pad"], c["off"]
    lddy, lddx, lds, lddr = N + pad, K + pad, K + 32 - pad, K + 16
    dyb, dyp = inp(o["dy"], dt, lddy, off)
    Wg = _w(o["W"], dt)
    sb, sp = inp(o["saved"], dt, lds, off) if o.get("saved") is not None else (None, None)
    rb, rp = inp(o["dres"], dt, lddr, off) if o.get("dres") is not None else (None, None)
    dx = Out(dt, M, K, lddx, off)
    name = f"mivit_{c['fam']}_dgrad"
    N_.check(_fn(name, dt if c["fam"] != "gemm_dma" else "bf16")(dyp, lddy, _p(Wg), M, N, K, c.get("dact", 0), sp, lds if sp else 0,
                                                                   rp, lddr if rp else 0, dx.ptr, lddx, _st()), name)
    torch.cuda.synchronize()
    return dx.read()


def _ws(nbytes):
    return torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")        # NaN patterns; 256 guard bytes behind


def _ws_guard_ok(ws, nbytes):
    return bool((ws[nbytes:] == 0xFF).all())


def run_wgrad(c, dt, o):
    """-> (dW, db) of two calls, asserted bitwise equal (fixed-order slab reduction)"""
    N_ = _N()
    M, N, K = c["M"], c["N"], c["K"]
    pad, off = c["pad"], c["off"]
    lddy, ldx = N + pad, K + 32 - pad
    dyb, dyp = inp(o["dy"], dt, lddy, off)
    xb, xp = inp(o["x"], dt, ldx, off)
    nbytes = _fn(f"mivit_{c['fam']}_workspace_bytes", dt)(M, N, K)
    assert nbytes == (sc.wgrad_dma_ws_bytes(M, N, K) if c["fam"] == "wgrad_bf16" else sc.small_ws_bytes(N, K))
    res = []
    for _ in range(2):
        ws, dW = _ws(nbytes), Out("f32", N, K, K)
        db = None if c.get("nodb") else Out("f32", 1, N, N)
        N_.check(_fn(f"mivit_{c['fam']}", dt)(dyp, lddy, xp, ldx, M, N, K, dW.ptr, db.ptr if db else None, _p(ws), nbytes, _st()),
                 c["fam"])
        torch.cuda.synchronize()
        assert _ws_guard_ok(ws, nbytes), "the kernel wrote behind its workspace"
        res.append((dW.read(), db.read()[0] if db else None))
    for a, b in zip(*res):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32)), "wgrad is not repeatable"
    return res[0]


def run_embed(c, dt, o, fwd=True, wgrad=True):
    """-> (y, dW, db): the fp32-frame embedding forward and weight gradient (db: small frames only)"""
    N_ = _N()
    M, E, K = c["M"], c["N"], c["K"]
    small = c["fam"] == "embed_small"
    xb, xp = inp(o["x"], "f32", K, c.get("off", 0))
    Wg, bg = _w(o["W"], dt), o["bias"].cuda()
    y = dW = db = None
    if fwd:
        yo = Out(dt, M, E, E)
        name = "mivit_embed_small_fwd" if small else "mivit_embed_fwd_bf16"
        N_.check(_fn(name, dt)(xp, _p(Wg), _p(bg), M, K, E, yo.ptr, _st()), name)
        torch.cuda.synchronize()
        y = yo.read()
    if wgrad:
        dyb, dyp = inp(o["dy"], dt, E, 0)
        res = []
        for _ in range(2):
            dWo = Out("f32", E, K, K)
            if small:
                nbytes = _fn("mivit_embed_small_wgrad_workspace_bytes", dt)(M, K, E)
                assert nbytes == sc.small_ws_bytes(E, K)
                ws, dbo = _ws(nbytes), Out("f32", 1, E, E)
                N_.check(_fn("mivit_embed_small_wgrad", dt)(dyp, xp, M, K, E, dWo.ptr, dbo.ptr, _p(ws), nbytes, _st()), "embed_small_wgrad")
            else:
                nbytes = _fn("mivit_embed_wgrad_bf16_workspace_bytes", dt)(M, K, E)
                assert nbytes == sc.embed_wgrad_ws_bytes(M, K, E)
                ws, dbo = _ws(nbytes), None
                N_.check(_fn("mivit_embed_wgrad_bf16", dt)(dyp, xp, M, K, E, dWo.ptr, _p(ws), nbytes, _st()), "embed_wgrad")
            torch.cuda.synchronize()
            assert _ws_guard_ok(ws, nbytes), "the kernel wrote behind its workspace"
            res.append((dWo.read(), dbo.read()[0] if dbo else None))
        for a, b in zip(*res):
            assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32)), "embed wgrad is not repeatable"
        dW, db = res[0]
    return y, dW, db


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------
def _ln_check(ep, dt, what, c, o, r):
    """the fused LayerNorm on the z the kernel stored"""
    z = r["y"].float()
    ref64, ref32 = sc.ref_ln(z, o["gamma"], o["beta"]), sc.ref_ln(z, o["gamma"], o["beta"], cdt=torch.float32)
    for name, got, a64, a32, out_dt in zip(("ln_out", "mean", "rstd"), (r["ln"], r["mean"], r["rstd"]), ref64, ref32, (dt, "f32", "f32")):
        yard = oc.yardstick(a32, a64)
        _check(ep, dt, f"{what} {name}", got, a64, oc.measured_bar(a64, yard, out_dt))


def _fwd_bars(c, dt, o):
    x, W = o["x"], o["W"]
    y64, u64 = sc.ref_fwd(dt, x, W, o.get("bias"), c.get("act", 0), o.get("resid"))
    term = oc.gemm_fp32_term(oc.rnd(x, dt), oc.rnd(W, dt).t(), c["K"], 2.0)
    bar_y = oc.half_ulp(y64, dt) + term
    if c.get("act") == 3:
        y32 = sc.ref_fwd(dt, x, W, o.get("bias"), 3, o.get("resid"), cdt=torch.float32)[0]
        bar_y = bar_y + 4 * oc.yardstick(y32, y64) * y64.abs().amax(-1, keepdim=True)
    return y64, u64, bar_y, oc.half_ulp(u64, dt) + term


def _dgrad_bar(c, dt, o):
    d64 = sc.ref_dgrad(dt, o["dy"], o["W"], c.get("dact", 0), o.get("saved"), o.get("dres"))
    bar = oc.half_ulp(d64, dt) + oc.gemm_fp32_term(o["dy"], oc.rnd(o["W"], dt), c["N"], 2.0)
    if c.get("dact") == 3:
        d32 = sc.ref_dgrad(dt, o["dy"], o["W"], 3, o["saved"], o.get("dres"), cdt=torch.float32)
        bar = bar + 4 * oc.yardstick(d32, d64) * d64.abs().amax(-1, keepdim=True)
    return d64, bar


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt,c", _params(sc.FAMILY_CASES))
def test_forward_and_dgrad_exact(dt, c, switches):
    _apply_switches(switches, c, dt)
    o = sc.int_operands(c)
    if c["kind"] == "fwd":
        r = run_fwd(c, dt, o)
        y64, u64 = sc.ref_fwd(dt, o["x"], o["W"], o.get("bias"), c.get("act", 0), o.get("resid"))
        assert torch.equal(r["y"].double(), y64), "y"
        if c.get("pre"):
            assert torch.equal(r["pre"].double(), u64), "y_preact"
        if c.get("ln"):
            _ln_check(f"{c['fam']}_fwd", dt, c["id"], c, o, r)
    else:
        dx = run_dgrad(c, dt, o)
        assert torch.equal(dx.double(), sc.ref_dgrad(dt, o["dy"], o["W"], c.get("dact", 0), o.get("saved"), o.get("dres"))), "dx"


@gpu
@pytest.mark.parametrize("dt", sc.H16)
def test_default_mode_equals_the_mode_ws_pick_names(dt, switches):
    """with nothing set the entry runs what the restated ws_pick says: bitwise the result of mode 1 where it picks wave-stream,
    of mode 0 where it does not (random data: the two kernels' fp32 summation orders need not agree, the pick must)"""
    N_ = _N()
    assert _fn("mivit_rowstream_set_wavestream", dt)(2) == 2 and _fn("mivit_rowstream_set_wavestream_mask", dt)(7) == 7
    for c in [sc._mk("rowstream", "fwd", 319, 128, 128, 0, ln=True), sc._mk("rowstream", "fwd", 319, 128, 128, 1, resid=True),
              sc._mk("rowstream", "dgrad", 319, 128, 128, 0, dact=1), sc._mk("rowstream", "dgrad", 319, 256, 256, 1, resid=True),
              sc._mk("rowstream", "dgrad", 319, 128, 384, 0)]:
        o = sc.rand_operands(c, dt, seed=3)
        run = (lambda: run_fwd(c, dt, o)["y"]) if c["kind"] == "fwd" else (lambda: run_dgrad(c, dt, o))
        default = run()
        NC, KC = sc.gemm_dims(c)
        pick = sc.ws_pick(2, 7, NC, KC, c["kind"] == "dgrad", bool(c.get("ln")), bool(c.get("dact")))
        switches("mivit_rowstream_set_wavestream", dt, 1 if pick else 0)
        assert torch.equal(default.view(torch.int16), run().view(torch.int16)), c["id"]
        switches("mivit_rowstream_set_wavestream", dt, 2)


@gpu
@pytest.mark.parametrize("dt,c", _params(sc.WGRAD_CASES))
def test_wgrad_exact(dt, c, switches):
    _apply_switches(switches, c, dt)
    o = sc.int_operands(c)
    dW, db = run_wgrad(c, dt, o)
    rW, rb = sc.ref_wgrad(dt, o["dy"], o["x"])
    assert torch.equal(dW.double(), rW), "dW"
    assert c.get("nodb") or torch.equal(db.double(), rb), "db"


@gpu
@pytest.mark.parametrize("dt,c", _params(sc.EMBED_SMALL_CASES + sc.EMBED_LARGE_CASES))
def test_embedding_exact(dt, c, switches):
    _apply_switches(switches, c, dt)
    small = c["fam"] == "embed_small"
    if small:
        assert _fn("mivit_embed_small_supported", dt)(c["M"], c["K"], c["N"]) == 1
    o = sc.int_operands(c)
    y, dW, db = run_embed(c, dt, o, fwd=not c.get("wgrad_only"), wgrad=not c.get("fwd_only"))
    if y is not None:
        assert torch.equal(y.double(), sc.ref_fwd(dt, o["x"], o["W"], o["bias"], 0, None)[0]), "y"
    if dW is not None:
        rW, rb = sc.ref_wgrad(dt, o["dy"], o["x"])
        assert torch.equal(dW.double(), rW), "dW"
        assert db is None or torch.equal(db.double(), rb), "db"


# ---------------------------------------------------------------------------------------------------------------------
# accuracy cases
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt,c", _params(sc.ACCURACY_CASES))
def test_forward_and_dgrad_accuracy(dt, c, switches):
    _apply_switches(switches, c, dt)
    o = sc.rand_operands(c, dt)
    ep = f"{c['fam']}_{c['kind']}"
    if c["kind"] == "fwd":
        r = run_fwd(c, dt, o)
        y64, u64, bar_y, bar_u = _fwd_bars(c, dt, o)
        _check(ep, dt, c["id"] + " y", r["y"], y64, bar_y)
        if c.get("pre"):
            _check(ep, dt, c["id"] + " y_preact", r["pre"], u64, bar_u)
        if c.get("ln"):
            _ln_check(ep, dt, c["id"], c, o, r)
    else:
        d64, bar = _dgrad_bar(c, dt, o)
        _check(ep, dt, c["id"], run_dgrad(c, dt, o), d64, bar)


_WG_RANDOM = [sc._wg("wgrad_bf16", 319, 128, 256, 0, cfg=0), sc._wg("wgrad_bf16", 1007, 256, 128, 1, cfg=31),
              sc._wg("wgrad_small", 271, 192, 64, 0), sc._wg("wgrad_small", 1057, 64, 128, 1)]


@gpu
@pytest.mark.parametrize("dt,c", _params(_WG_RANDOM))
def test_wgrad_accuracy_and_determinism(dt, c, switches):
    _apply_switches(switches, c, dt)
    o = sc.rand_operands(c, dt)
    dW, db = run_wgrad(c, dt, o)                                  # two calls inside, bitwise equal
    rW, rb = sc.ref_wgrad(dt, o["dy"], o["x"])
    slabs = sc.wgrad_dma_splits(c["M"], c["N"], c["K"])[1] if c["fam"] == "wgrad_bf16" else 256
    _check(c["fam"], dt, c["id"] + " dW", dW, rW, oc.gemm_fp32_term(o["dy"].t(), o["x"], c["M"] + slabs))
    _check(c["fam"], dt, c["id"] + " db", db, rb, (c["M"] + slabs) * oc.U32 * o["dy"].abs().double().sum(0))


_EMB_RANDOM = [sc._c(id="embed_small-257x64x81", fam="embed_small", kind="embed", M=257, N=64, K=81, off=1),
               sc._c(id="embed_small-1057x128x169", fam="embed_small", kind="embed", M=1057, N=128, K=169, off=1),
               sc._c(id="embed_large-131x128x384", fam="embed_large", kind="embed", M=131, N=128, K=384, variant=0),
               sc._c(id="embed_large-1031x128x256", fam="embed_large", kind="embed", M=1031, N=128, K=256, variant=0)]


@gpu
@pytest.mark.parametrize("dt,c", _params(_EMB_RANDOM))
def test_embedding_accuracy_and_determinism(dt, c, switches):
    _apply_switches(switches, c, dt)
    o = sc.rand_operands(c, dt)
    y, dW, db = run_embed(c, dt, o)
    y64 = sc.ref_fwd(dt, o["x"], o["W"], o["bias"], 0, None)[0]
    _check(c["fam"] + "_fwd", dt, c["id"], y, y64, oc.half_ulp(y64, dt) + oc.gemm_fp32_term(oc.rnd(o["x"], dt), o["W"].t(), c["K"], 2.0))
    rW, rb = sc.ref_wgrad(dt, o["dy"], o["x"])
    slabs = 256
    _check(c["fam"] + "_wgrad", dt, c["id"] + " dW", dW, rW, oc.gemm_fp32_term(o["dy"].t(), oc.rnd(o["x"], dt), c["M"] + slabs))
    if db is not None:
        _check(c["fam"] + "_wgrad", dt, c["id"] + " db", db, rb, (c["M"] + slabs) * oc.U32 * o["dy"].abs().double().sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _fwd_call(fam, dt, M, N, K, ldx=None, xoff=0, ldy=None, yoff=0, ldr=None, roff=0, resid=False, ln=False, N_ln=None):
    """-> (rc, y Out): a forward call on zero operands with one thing wrong; the output must come back untouched"""
    ldx, ldy, ldr = ldx or K, ldy or N, ldr or N
    x = torch.zeros(M * ldx + 16, dtype=DT[dt], device="cuda")
    W = torch.zeros(N * K, dtype=DT[dt], device="cuda")
    b = torch.zeros(N, device="cuda")
    r = torch.zeros(M * ldr + 16, dtype=DT[dt], device="cuda") if (resid or ln) else None
    y = Out(dt, M, N, ldy, yoff)
    args = [x.data_ptr() + 2 * xoff, ldx, _p(W), _p(b), M, N, K, 0, (r.data_ptr() + 2 * roff) if r is not None else None, ldr,
            y.ptr, ldy, None]
    keep = [x, W, b, r]
    if fam != "gemm_dma":
        if ln:
            g = torch.ones(N, device="cuda")
            lo, mu, rs = Out(dt, M, N, N), Out("f32", 1, M, M), Out("f32", 1, M, M)
            args += [_p(g), _p(g), lo.ptr, mu.ptr, rs.ptr]
            keep += [g, lo, mu, rs]
        else:
            args += [None] * 5
    rc = _fn(f"mivit_{fam}_fwd", dt if fam != "gemm_dma" else "bf16")(*args, _st())
    torch.cuda.synchronize()
    return rc, y, keep


def _untouched(y):
    flat = y.raw.cpu()
    return bool((flat == SENT[ESIZE[y.dt]]).all())


@gpu
@pytest.mark.parametrize("dt", sc.H16)
@pytest.mark.parametrize("fam", ["rowstream", "wavestream"])
def test_refusals_forward(fam, dt, switches):
    N_ = _N()
    if fam == "rowstream":
        switches("mivit_rowstream_set_wavestream", dt, 0)
    bad_k = 192 if fam == "rowstream" else 96
    for what, kw in (("M = 255", dict(M=255)), ("unsupported K", dict(K=bad_k)), ("unsupported N", dict(N=96)),
                     ("ldx % 8", dict(ldx=132)), ("x 2 bytes off", dict(xoff=1))):
        a = dict(M=256, N=128, K=128)
        a.update(kw)
        rc, y, _ = _fwd_call(fam, dt, **a)
        assert rc == 3 and _untouched(y), (what, rc)
        assert "unsupported" in N_.last_error()
    for what, kw in (("ldy % 8", dict(ldy=132)), ("y 2 bytes off", dict(yoff=1)), ("ldr % 8", dict(resid=True, ldr=132)),
                     ("resid 2 bytes off", dict(resid=True, roff=1)), ("LayerNorm with N != BN", dict(N=256, ln=True))):
        a = dict(M=256, N=128, K=128)
        a.update(kw)
        rc, y, _ = _fwd_call(fam, dt, **a)
        assert rc not in (0, 3) and _untouched(y), (what, rc)
        assert fam in N_.last_error(), (what, N_.last_error())
    # fused LayerNorm without a residual
    M, N, K = 256, 128, 128
    x, W, g = (torch.zeros(M * K, dtype=DT[dt], device="cuda"), torch.zeros(N * K, dtype=DT[dt], device="cuda"), torch.ones(N, device="cuda"))
    y, lo, mu, rs = Out(dt, M, N, N), Out(dt, M, N, N), Out("f32", 1, M, M), Out("f32", 1, M, M)
    rc = _fn(f"mivit_{fam}_fwd", dt)(_p(x), K, _p(W), None, M, N, K, 0, None, 0, y.ptr, N, None, _p(g), _p(g), lo.ptr, mu.ptr, rs.ptr, _st())
    torch.cuda.synchronize()
    assert rc not in (0, 3) and "LayerNorm" in N_.last_error() and _untouched(y) and _untouched(lo)


@gpu
def test_refusals_gemm_dma():
    N_ = _N()
    for kw in (dict(M=255), dict(K=96), dict(N=192), dict(K=160)):
        a = dict(M=256, N=128, K=128)
        a.update(kw)
        rc, y, _ = _fwd_call("gemm_dma", "bf16", **a)
        assert rc == 3 and _untouched(y), kw
        assert N_.lib.mivit_gemm_dma_supported(a["M"], a["N"], a["K"], 0) == 0
    for kw in (dict(ldx=132), dict(xoff=1), dict(ldy=132), dict(yoff=1), dict(resid=True, ldr=132), dict(resid=True, roff=1)):
        rc, y, _ = _fwd_call("gemm_dma", "bf16", M=256, N=128, K=128, **kw)
        assert rc not in (0, 3) and "aligned" in N_.last_error() and _untouched(y), kw


@gpu
@pytest.mark.parametrize("dt", sc.H16)
@pytest.mark.parametrize("fam", ["wgrad_bf16", "wgrad_small"])
def test_refusals_wgrad(fam, dt):
    N_ = _N()
    M, N, K = (256, 128, 128) if fam == "wgrad_bf16" else (256, 64, 64)

    def call(M=M, N=N, K=K, lddy=None, ldx=None, dyoff=0, short=0):
        lddy, ldx = lddy or N, ldx or K
        dy = torch.zeros(M * lddy + 16, dtype=DT[dt], device="cuda")
        x = torch.zeros(M * ldx + 16, dtype=DT[dt], device="cuda")
        nbytes = max(_fn(f"mivit_{fam}_workspace_bytes", dt)(M, N, K), 256)
        ws, dW, db = _ws(nbytes), Out("f32", N, K, K), Out("f32", 1, N, N)
        rc = _fn(f"mivit_{fam}", dt)(dy.data_ptr() + 2 * dyoff, lddy, _p(x), ldx, M, N, K, dW.ptr, db.ptr, _p(ws), nbytes - short, _st())
        torch.cuda.synchronize()
        assert _untouched(dW) and _untouched(db) and bool((ws == 0xFF).all())
        return rc
    assert call(M=255) == 3 and call(N=N + 32 if fam == "wgrad_bf16" else 80) == 3 and call(lddy=N + 4) == 3
    assert call(ldx=K + 4) == 3 and call(dyoff=1) == 3
    assert "unsupported" in N_.last_error()
    rc = call(short=1)
    assert rc not in (0, 3) and "workspace too small" in N_.last_error()


@gpu
@pytest.mark.parametrize("dt", sc.H16)
def test_embed_small_supported_agrees_with_the_entries(dt):
    for M, K, E in ((256, 81, 64), (255, 81, 64), (256, 257, 64), (256, 0 + 300, 128), (256, 81, 96), (300, 256, 128), (256, 1, 64)):
        want = int(sc.embed_small_supported(M, K, E))
        assert _fn("mivit_embed_small_supported", dt)(M, K, E) == want
        x = torch.zeros(M * K, device="cuda")
        W, b = torch.zeros(E * K, dtype=DT[dt], device="cuda"), torch.zeros(E, device="cuda")
        dy = torch.zeros(M * E, dtype=DT[dt], device="cuda")
        y, dW, db = Out(dt, M, E, E), Out("f32", E, K, K), Out("f32", 1, E, E)
        rc = _fn("mivit_embed_small_fwd", dt)(_p(x), _p(W), _p(b), M, K, E, y.ptr, _st())
        nbytes = max(_fn("mivit_embed_small_wgrad_workspace_bytes", dt)(M, K, E), 256)
        ws = _ws(nbytes)
        rc2 = _fn("mivit_embed_small_wgrad", dt)(_p(dy), _p(x), M, K, E, dW.ptr, db.ptr, _p(ws), nbytes, _st())
        torch.cuda.synchronize()
        assert (rc, rc2) == ((0, 0) if want else (3, 3)), (M, K, E, rc, rc2)
        if want:
            assert float(y.read().float().abs().max()) == 0 and float(dW.read().abs().max()) == 0
        else:
            assert _untouched(y) and _untouched(dW) and _untouched(db)
