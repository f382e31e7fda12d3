"""CPU: the references, dispatch restatements and case tables of tests/streaming_common.py.  A table that stops reaching a
kernel instantiation fails here; the GPU file (tests/test_streaming_ops_gpu.py) runs exactly these tables."""
import pytest
import torch

import operators_common as oc
import streaming_common as sc


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("dt", sc.H16)
def test_references_agree_with_autograd(dt, act):
    x, W = oc.randn((37, 64), 1, 1.0, dt), oc.randn((24, 64), 2, 0.125, dt)
    bias, resid, dy = oc.randn((24,), 3), oc.randn((37, 24), 4, 1.0, dt), oc.randn((37, 24), 5, 1.0, dt)
    worst = sc.autograd_check(dt, x, W, bias, act, resid, dy)
    assert max(worst) < 1e-12, worst
    # fused LayerNorm: the reference against torch's, on the stored sum
    z = oc.rnd(sc.ref_fwd(dt, x, W, bias, act, resid)[0], dt)
    g, b = 1 + 0.1 * oc.randn((24,), 6), oc.randn((24,), 7)
    y, mu, rs = sc.ref_ln(z, g, b)
    assert float((y - torch.nn.functional.layer_norm(z, (24,), g.double(), b.double(), oc.LN_EPS)).abs().max()) < 1e-12
    assert float((mu - z.mean(-1)).abs().max()) < 1e-13


def _instances(cases, fam=None):
    out = {dt: set() for dt in sc.H16}
    for c in cases:
        if fam and c["fam"] != fam:
            continue
        for dt in sc.case_dts(c):
            out[dt].add(sc.case_instance(c, dt))
    return out


def test_tables_reach_every_wavestream_and_rowstream_instantiation():
    got = _instances(sc.FAMILY_CASES)
    for dt in sc.H16:
        assert sc.REQUIRED_WS <= got[dt], (dt, sorted(sc.REQUIRED_WS - got[dt]))
        assert sc.REQUIRED_RS <= got[dt], (dt, sorted(sc.REQUIRED_RS - got[dt]))
    # the five instantiations behind the default picks: never under mode 2, each under mode 0; under mode 1 nothing with a
    # shape wave-stream supports runs a row-stream kernel
    by_mode = {m: {sc.case_instance(c, "bf16") for c in sc.FAMILY_CASES if c["fam"] == "rowstream" and c.get("ws_mode") == m}
               for m in (0, 1, 2)}
    assert sc.RS_BEHIND_PICKS <= by_mode[0] and not (sc.RS_BEHIND_PICKS & by_mode[2])
    assert {i for i in by_mode[1] if i[0] == "rs"} == {("rs", 384, True, False, ek) for ek in (0, 2, 3)}
    assert all(i[0] == "rs" for i in by_mode[0])
    # accuracy cases run real row-stream kernels too
    assert any(sc.case_instance(c, "bf16")[0] == "rs" for c in sc.ACCURACY_CASES)


def test_tables_reach_every_gemm_dma_variant():
    got = _instances(sc.FAMILY_CASES, "gemm_dma")["bf16"]
    assert sc.REQUIRED_GD <= got, sorted(sc.REQUIRED_GD - got)
    seen = {(c["variant"], c["kind"]) for c in sc.FAMILY_CASES if c["fam"] == "gemm_dma"}
    assert {(v, k) for v in sc.GD_VARIANTS for k in ("fwd", "dgrad")} <= seen
    # distinct kernels: 11 launch_t variants (7 doubles as the dgrad default, 6 as the forward default) + 5 + 5 transposed
    assert len(sc.REQUIRED_GD) == 2 * (11 + 5 + 5)
    for c in sc.FAMILY_CASES:
        NC, KC = sc.gemm_dims(c)
        if c["fam"] == "gemm_dma":
            assert sc.gemm_dma_supported(c["M"], NC, KC), c["id"]
            v = c["variant"]
            if v in (20, 22, 27, 30, 32, 37):
                assert NC % 256 == 0, c["id"]            # the variant's own shape precondition: no silent default


def test_tables_reach_wgrad_and_embedding_branches():
    cfgs = {sc.wgrad_dma_config(c["cfg"], c["N"], c["K"]) for c in sc.WGRAD_CASES if c["fam"] == "wgrad_bf16"}
    assert cfgs == {(2, 32), (2, 64), (3, 32), (3, 64)}
    assert {c["cfg"] for c in sc.WGRAD_CASES if c["fam"] == "wgrad_bf16"} == {0, 21, 22, 31, 32}
    assert {sc.wgrad_dma_config(0, c["N"], c["K"]) for c in sc.WGRAD_CASES if c.get("cfg") == 0} == {(2, 32), (2, 64)}
    assert any(sc.wgrad_dma_splits(c["M"], c["N"], c["K"])[1] > 1 for c in sc.WGRAD_CASES if c["fam"] == "wgrad_bf16")
    small = [c for c in sc.WGRAD_CASES if c["fam"] == "wgrad_small"]
    assert {(sc.window_of(c["N"], c["K"]), c["K"]) for c in small} == {(64, 64), (128, 64), (96, 64), (64, 128)}
    gx = [sc.small_grid_x(c["M"], c["N"] // sc.window_of(c["N"], c["K"])) for c in small]
    assert 1 in gx and any(g > 1 for g in gx)
    assert any(sc.cdiv(c["M"], 32) > g * 8 for c, g in zip(small, gx)), "no wave takes a second chunk"
    es = sc.EMBED_SMALL_CASES
    assert {(sc.frame_kp(c["K"]), c["N"]) for c in es} == {(kp, E) for kp in (64, 96, 128, 192, 256) for E in (64, 128)}
    assert {(c["K"], c["N"]) for c in es} >= {(K, E) for K in sc.SMALL_K for E in sc.SMALL_E}
    assert all(sc.embed_small_supported(c["M"], c["K"], c["N"]) for c in es)
    assert {sc.embed_fwd_instance(c["variant"], c["M"], c["N"]) for c in sc.EMBED_LARGE_CASES} == {
        ("dma", 128, 3), ("dma", 256, 2), ("dma32",), ("direct2", 2, 4, 3), ("direct", 2, 4, 3), ("direct", 1, 4, 2),
        ("direct", 1, 8, 3), ("direct", 1, 8, 2), ("direct", 2, 4, 2), ("direct", 1, 4, 3), ("direct", 1, 2, 3)}
    assert all(sc.embed_dma_supported(c["M"], c["K"], c["N"]) for c in sc.EMBED_LARGE_CASES)


def test_tables_have_a_second_tile_per_kernel():
    """one M per kernel just past the point where a workgroup (or wave) takes a second tile, from the restated grid rules"""
    def second(c):
        NC, KC = sc.gemm_dims(c)
        dg = c["kind"] == "dgrad"
        inst = sc.case_instance(c, "bf16")
        if inst[0] == "ws":
            return sc.cdiv(c["M"], 16) > sc.ws_grid_y(c["M"], NC, KC) * sc.ws_nwv(KC)
        if inst[0] == "rs":
            gy, BM = sc.rs_grid_y(c["M"], NC, KC, dg, inst[4] != 0)
            return sc.cdiv(c["M"], BM) > gy
        if inst[0] == "gd-pers":
            ntile, wgs = sc.gemm_pers_grid(c["M"], NC, inst[1:5])
            return ntile > wgs
        return False
    kinds = {sc.case_instance(c, "bf16")[0] for c in sc.FAMILY_CASES if second(c)}
    assert kinds == {"ws", "rs", "gd-pers"}, kinds
    assert {sc.case_instance(c, "bf16")[1] for c in sc.FAMILY_CASES if second(c) and c["fam"] == "rowstream"} == {128, 384}


def _all_int_cases():
    return sc.FAMILY_CASES + sc.WGRAD_CASES + sc.EMBED_SMALL_CASES + sc.EMBED_LARGE_CASES


@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in _all_int_cases()])
def test_integer_cases_are_exact_at_every_intermediate(c):
    """operands integers of bf16 (|v| <= 256 covers fp16 too), fp32 sums below 2^24, outputs exact in both element types; the
    LayerNorm outputs are not integers and are held to the accuracy bar instead"""
    o = sc.int_operands(c)
    for k, v in o.items():
        if v is not None and k not in ("gamma", "beta"):
            assert torch.equal(v, v.round()) and float(v.abs().max()) <= 16, k
    lim = sc.INT_LIMIT["bf16"]
    if c["kind"] == "fwd":
        y, u = sc.ref_fwd("bf16", o["x"], o["W"], o["bias"], c.get("act", 0), o.get("resid"))
        assert float((o["x"].abs().double() @ o["W"].abs().double().t()).max()) + 16 < 2 ** 24
        assert float(y.abs().max()) <= lim and float(u.abs().max()) <= lim, (float(y.abs().max()), float(u.abs().max()))
    elif c["kind"] == "dgrad":
        dx = sc.ref_dgrad("bf16", o["dy"], o["W"], c.get("dact", 0), o.get("saved"), o.get("dres"))
        assert float((o["dy"].double() @ o["W"].double()).abs().max()) <= lim and float(dx.abs().max()) <= lim
    else:
        dW, db = sc.ref_wgrad("bf16", o["dy"], o["x"])
        assert float((o["dy"].abs().double().t() @ o["x"].abs().double()).max()) < 2 ** 24 and float(db.abs().max()) < 2 ** 24
        if c["kind"] == "embed":
            y, _ = sc.ref_fwd("bf16", o["x"], o["W"], o["bias"], 0, None)
            assert float(y.abs().max()) <= lim


def test_print_yardsticks():
    """the fp32 yardsticks behind the GELU and LayerNorm bars (each GPU test uses the one of its own inputs)"""
    worst = {}
    for c in sc.ACCURACY_CASES:
        if c["M"] > 600:
            continue
        for dt in sc.case_dts(c):
            o = sc.rand_operands(c, dt)
            if c["kind"] == "fwd" and c.get("act") == 3:
                r64 = sc.ref_fwd(dt, o["x"], o["W"], o["bias"], 3, o.get("resid"))[0]
                r32 = sc.ref_fwd(dt, o["x"], o["W"], o["bias"], 3, o.get("resid"), cdt=torch.float32)[0]
                key = ("gelu fwd", dt)
            elif c["kind"] == "dgrad" and c.get("dact") == 3:
                r64 = sc.ref_dgrad(dt, o["dy"], o["W"], 3, o["saved"], o.get("dres"))
                r32 = sc.ref_dgrad(dt, o["dy"], o["W"], 3, o["saved"], o.get("dres"), cdt=torch.float32)
                key = ("gelu dgrad", dt)
            elif c.get("ln"):
                z = oc.rnd(sc.ref_fwd(dt, o["x"], o["W"], o["bias"], 0, o["resid"])[0], dt)
                for name, a, b in zip(("ln_out", "mean", "rstd"), sc.ref_ln(z, o["gamma"], o["beta"], cdt=torch.float32),
                                      sc.ref_ln(z, o["gamma"], o["beta"])):
                    worst[(name, dt)] = max(worst.get((name, dt), 0), oc.yardstick(a, b))
                continue
            else:
                continue
            worst[key] = max(worst.get(key, 0), oc.yardstick(r32, r64))
    for k, v in sorted(worst.items()):
        print(f"[streaming] yardstick {k[0]:10s} {k[1]:4s} {v:.2e}")
        assert oc.U32 <= v < 1e-4
