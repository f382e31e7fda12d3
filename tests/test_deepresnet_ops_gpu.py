"""The DeepResNet embedding kernels at the C-ABI -- mivit_deepresnet_train_fwd / _bwd (+ their staged forms),
mivit_deepresnet_infer (csrc/deepresnet_train.hip) and mivit_deepresnet_eval_fwd (csrc/deepresnet.hip) -- launch by launch
against fp64 arithmetic on the bytes each launch read (tests/deepresnet_common.py).

Rounding model (T = compute type, rnd = rounding to T; line numbers in csrc/deepresnet_train.hip):
  * conv0 (:547-582): fp32 frames x fp32 weights on the VALU; y0 = rnd(v); the statistics take the fp32 v (:573).
  * every MFMA convolution: the operand is computed in fp32 from the stored y and the fp32 table and ROUNDED TO T when it
    is staged into LDS (fill_batched :193-200 -> store16); weights are rnd(W) (drn_pack_kernel :1003-1010); accumulation in
    fp32; y = rnd(acc) (store4 :337-345).  The batch statistics are summed from the fp32 ACCUMULATORS, not from the rounded
    y (:423-429), per workgroup in fp32, then in fp64 (drn_bn_finalize_kernel :669-695; beyond 128 partials
    drn_part_reduce_kernel :707-719 sums in fp64 and rounds to fp32 once).  var = E[x^2] - mean^2 in fp64 from those sums.
  * pooling (:734-770) and the Linear: fp32.  Backward: g = rnd(upstream * [act > 0]) with act evaluated in fp32 on the
    stored y (:811-819, :405-417); the sums s = sum g, sum g*y take the unrounded fp32 g; tables [k|c0|c1], dgamma, dbeta in
    fp64 from the fp32 partials (:836-864); dy = k*g + c0 + c1*y in fp32, rounded to T when staged (weight gradient
    :919-920, data gradient :489); the first convolution's weight gradient keeps dy in fp32 (:634).  The data gradient of a
    block input is two passes: the 3x3 pass stores rnd(t), the 1x1 skip pass reads it back (:513-526): two roundings.
Bars (none tuned): half an ulp of T at the element (0 in fp32 mode) + fp32 accumulation K_red * 2^-24 * (|A| (*) |W|) on
the staged operands + the boundary term: an operand may be the other neighbour of T only where its fp64 value is within
its fp32 error (n_ops * 2^-24 * sum of |terms|) of a rounding boundary, and a ReLU may flip only within that error of
zero; that per-element uncertainty goes through |W| into the bar.  Statistics: the fp32 partial sums are no deeper than 32
(MFMA epilogue) / 68 (conv0, mask kernel) additions, so sum x and sum x^2 are good to that many units of sum |x|, sum x^2,
plus the convolution's own bar summed; the variance bar is that error of E[x^2] and mean^2 against var, carried exactly
through 1/sqrt (interval), scale and shift.  dgamma = rstd * (sum g y - mean * sum g) likewise.  Elements whose bar is
dominated by the boundary term stay checked against it; their share per tensor is capped at 5 % (weight gradients of the
P = 1, P = 2 and adversarial cases: the caps and the reasons in deepresnet_common.share_cap) and asserted, on the CPU from
the reference alone and here.
Single call: the forward is checked from the one call; the backward overwrites g2 and g21, which the reference
regenerates in fp64 with their rounding uncertainty carried through |W| (Walk `regen`), every other output as staged.
Fused inference kernel: nothing between frames and tokens is observable, so every activation's uncertainty is carried
through the five layers; the test folds BatchNorm in fp64 and rounds the weights itself.

Measured on the MI355X, worst error / bar over all cases (boundary-dominated share of that tensor in brackets where not 0):
  quantity        staged f32  staged bf16     single f32  single bf16    infer f32  infer bf16
  y1..y6          0.429       1.000           0.429       1.000          0.429      1.000
  fco tables      0.527       0.527           0.527       0.527          0.390      0.390
  running mean    0.261       0.261           0.261       0.261          -          -
  running var     0.232       0.213           0.232       0.213          -          -
  pooled          0.167       0.131           0.167       0.131          0.204      0.156
  tokens          0.013       0.012           0.013       0.012          0.016      0.019
  dpooled         0.331       0.331           0.331       0.331
  fc weight/bias  0.154/0.117 0.161/0.117     0.154/0.117 0.161/0.117
  g2..g0          0.467       1.000           0.018       0.982    (single: g1, g11, g0 only)
  bco tables      0.495       0.490           0.495       0.490
  dgamma          0.045       0.334           0.045       0.334
  dbeta           0.066       0.414           0.066       0.414
  dW0..dW6        0.014       0.899 [0.065]   0.033       0.713 [0.010]
In bf16 a stored tensor's bar is almost all final rounding, so 1.000 says the worst element sat next to a rounding
boundary; the fp32 column shows how much of the arithmetic term is used.  Boundary-dominated shares on the kernels' own
values stay under the caps of deepresnet_common.share_cap (worst: dW4 of P2-N75, 0.065 of a cap of 0.10); in fp32 mode the
share is 0 by construction.  eval_fwd tokens: below 0.001 of the bar in both dtypes (every bf16 token boundary-dominated):
the uncertainty carried through five unobservable layers by |W| is a worst case that is far from attained, so this check
catches gross faults of the fused kernel only (placement, a missing layer or bias), not a subtly wrong sum.
All 83 GPU cases take 16 s including start-up, the 26 training cases 6.3 s, the slowest (f32-whole-9x9-ragged, the first
to touch the library) 1.3 s.
Cancellation (issue section 4), measured against fp64, in fp32 roundings (2^-24 relative):
  * camera counts (DC 5000 + spot): BatchNorm 0 has E[x^2] / var = 12 and its rstd is off by 17 roundings (var by 34); the
    six MFMA layers see normalised inputs (E[x^2] / var 1.3 .. 7) and are off by 1.5 .. 5 roundings.  No digits of
    consequence are lost at camera-count scale: the spot makes the first layer's variance large.
  * the adversarial channel (var 9.8e-7, E[x^2] / var 1.0e6): rstd is off by 2.4e4 roundings (1.4e-3 relative), i.e. the
    variance by 5.4e5 roundings, 3.2 % of itself -- E[x^2] - mean^2 from fp32 per-workgroup sums keeps 24 bits of E[x^2],
    not of var, and loses log2(E[x^2] / var) = 20 of them.  With eps = 1e-5 ten times the variance the effect on the
    normalised activation is 1.4e-3.  This is the documented limit of the summation; the bar follows it (0.527 used).
  * dgamma = rstd * (sum g y - mean * sum g), fp32 mode, relative to |dgamma| itself: 60 .. 2600 roundings (1.6e-4 at
    worst, BatchNorm 5 of the camera-count case); against the derived bar 0.045.  In bf16 mode the operands' rounding to T
    dominates and a dgamma that cancels to nearly zero can be off by a fifth of itself (0.334 of its bar).
Mutations of csrc/deepresnet_train.hip tried in a scratch copy (never committed), each against the small training cases:
  * wrong halo source for the last tile column (cell_source: the left halo cell of the last tile column reads one pixel to
    the right): the 5 tiled cases fail (f32 divides-10, overhang-13, three-tiles-19, bf16 divides-14,
    three-tiles-overhang-29), the 13 whole-frame cases pass; worst y0 3.7e6, y1 2.0e4, dW1 1.4e4, g11 8.8e3 of the bar.
  * one tap dropped (drn_pack_kernel zeroes tap 8 of the forward pack): 16 of 18 fail, y1 2.4e4, y2 8.2e3, y4 7.9e3, y5
    2.7e3 of the bar; the two P = 1 cases pass, where tap 8 only ever meets zero padding.
  * `count - 1` in the mean (drn_bn_finalize_kernel): 18 of 18 fail, fco0 8.7e3, running mean 8.0e3, running var 4.4e3 of
    the bar.
Memory: workspaces of exactly the queried size with a sentinel guard, guards around tokens and every gradient, frames
inside a NaN-padded allocation; NaN bit patterns in the workspace before the first call.
"""
import ctypes
import os
import re
import subprocess
import sys
import time

import pytest
import torch

import deepresnet_common as dc

gpu = pytest.mark.gpu
SENT = 0x7FC0BEEF
GUARD = 64                      # int32 elements = 256 bytes
_WORST, _TIMES = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (ep, dt, name), (ratio, share, cid) in sorted(_WORST.items()):
        print(f"[deepresnet] {ep:12s} {dt:4s} {name:8s} worst error/bar {ratio:.3f}  boundary share {share:.4f}  ({cid})")
    if _TIMES:
        k = max(_TIMES, key=_TIMES.get)
        print(f"[deepresnet] slowest case {k} {_TIMES[k]:.2f} s, total {sum(_TIMES.values()):.1f} s")


def _N():
    from moleculardiffusion_mivit_amd import _native as N
    return N


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """fp32 device buffer with a sentinel guard before and after, checked bitwise by read()"""

    def __init__(self, n, init=None, fill=SENT):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32)
        self.raw[GUARD:GUARD + n] = fill if init is None else init.float().reshape(-1).view(torch.int32)
        self.raw = self.raw.cuda()
        self.ptr = self.raw.data_ptr() + GUARD * 4

    def read(self):
        assert bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.n:] == SENT).all()), "write outside the buffer"
        return self.raw[GUARD:GUARD + self.n].view(torch.float32)


class Problem:
    def __init__(self, dt, c, prm=None, running=None):
        N_ = _N()
        self.dt, self.c, self.N, self.P, self.E = dt, c, c["N"], c["P"], c["E"]
        self.momentum = c.get("momentum", 0.1)
        p32, x, dtok = dc.case_inputs(c)
        self.p32 = p32
        self.dev = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in p32.items()}
        self.running = c.get("running", True) if running is None else running
        self.prm = dc.to64(p32, "cuda")
        R = self.N * self.P * self.P
        xb = torch.full((R + 2 * GUARD,), float("nan"))
        xb[GUARD:GUARD + R] = x.reshape(-1)
        self.xbuf = xb.cuda()
        self.xptr = self.xbuf.data_ptr() + GUARD * 4
        self.x64, self.dtok64 = x.double().cuda(), dtok.double().cuda()
        self.dtok = dtok.cuda()
        self.code = dc.CODE[dt]
        self.bytes = N_.lib.mivit_deepresnet_train_workspace_bytes(self.code, self.N, self.P, self.E)
        assert self.bytes == dc.ws_layout(dt, self.N, self.P, self.E)[15]
        self.off = dc.ws_layout(dt, self.N, self.P, self.E)
        self.fresh()

    def fresh(self, pass_running=None):
        """new workspace (NaN patterns + guard), outputs, running statistics and parameter struct"""
        pass_running = self.running if pass_running is None else pass_running
        N_ = _N()
        self.ws = torch.full((self.bytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        self.ws[self.bytes:] = 0xA5
        assert self.ws.data_ptr() % 256 == 0
        self.rm = [Guarded(dc.CO[i], self.p32["rm"][i]) for i in range(7)]
        self.rv = [Guarded(dc.CO[i], self.p32["rv"][i]) for i in range(7)]
        self.params = N_.DeepResNetParams()
        for i in range(7):
            cb = self.params.conv[i]
            cb.weight, cb.gamma, cb.beta = self.dev["W"][i].data_ptr(), self.dev["gamma"][i].data_ptr(), self.dev["beta"][i].data_ptr()
            cb.running_mean = self.rm[i].ptr if pass_running else None
            cb.running_var = self.rv[i].ptr if pass_running else None
        self.params.fc_weight, self.params.fc_bias = self.dev["fcw"].data_ptr(), self.dev["fcb"].data_ptr()
        self.tokens = Guarded(self.N * self.E)
        self.gW = [Guarded(dc.CO[i] * dc.CI[i] * dc.TAPS[i]) for i in range(7)]
        self.gG = [Guarded(dc.CO[i]) for i in range(7)]
        self.gB = [Guarded(dc.CO[i]) for i in range(7)]
        self.gfw, self.gfb = Guarded(self.E * 128), Guarded(self.E)
        self.grads = N_.DeepResNetGrads()
        for i in range(7):
            self.grads.conv[i].weight, self.grads.conv[i].gamma, self.grads.conv[i].beta = self.gW[i].ptr, self.gG[i].ptr, self.gB[i].ptr
        self.grads.fc_weight, self.grads.fc_bias = self.gfw.ptr, self.gfb.ptr
        self.stats = torch.zeros(2 * 3 * 128, dtype=torch.float64, device="cuda")
        self.count = torch.tensor([float(self.N * self.P * self.P)], dtype=torch.float64, device="cuda")

    # ---- calls ----
    def fwd(self, stage=None, infer=False):
        N_, a = _N(), (self.code, ctypes.byref(self.params), self.xptr, self.N, self.P, self.E)
        wsa = (self.tokens.ptr, self.ws.data_ptr(), self.bytes)
        if infer:
            rc = N_.lib.mivit_deepresnet_infer(*a, dc.EPS, *wsa, _st())
        elif stage is None:
            rc = N_.lib.mivit_deepresnet_train_fwd(*a, self.momentum, dc.EPS, *wsa, _st())
        else:
            rc = N_.lib.mivit_deepresnet_train_fwd_stage(*a, self.momentum, dc.EPS, *wsa, stage, self.count.data_ptr(),
                                                         self.stats.data_ptr(), _st())
        N_.check(rc, "deepresnet forward")

    def bwd(self, stage=None):
        N_ = _N()
        a = (self.code, ctypes.byref(self.params), self.xptr, self.dtok.data_ptr(), self.N, self.P, self.E, dc.EPS,
             ctypes.byref(self.grads), self.ws.data_ptr(), self.bytes)
        if stage is None:
            rc = N_.lib.mivit_deepresnet_train_bwd(*a, _st())
        else:
            rc = N_.lib.mivit_deepresnet_train_bwd_stage(*a, stage, self.count.data_ptr(), self.stats.data_ptr(), _st())
        N_.check(rc, "deepresnet backward")

    # ---- reading ----
    def region(self, k, n, f32=False):
        tdt = torch.float32 if f32 else dc.DT[self.dt]
        return self.ws[self.off[k]:self.off[k] + n * tdt.itemsize].view(tdt).double()

    def check_guard(self):
        torch.cuda.synchronize()
        assert bool((self.ws[self.bytes:] == 0xA5).all()), "write past the workspace"

    def got_forward(self, infer=False):
        self.check_guard()
        R = self.N * self.P * self.P
        got = {f"y{i}": self.region(i, R * dc.CO[i]).reshape(R, dc.CO[i]) for i in range(7)}
        ft = self.region(7, 7 * 4 * 128, True).reshape(7, 4, 128)
        for i in range(7):
            got[f"fco{i}"] = ft[i, :, :dc.CO[i]]
            rm, rv = self.rm[i].read().double(), self.rv[i].read().double()
            if self.running and not infer:
                got[f"rm{i}"], got[f"rv{i}"] = rm, rv
            else:                                            # untouched: NULL pointers were passed / inference
                assert torch.equal(rm, self.prm["rm"][i]) and torch.equal(rv, self.prm["rv"][i])
        got["pooled"] = self.region(9, self.N * 128, True).reshape(self.N, 128)
        got["tokens"] = self.tokens.read().double().reshape(self.N, self.E)
        return got

    def got_backward(self):
        self.check_guard()
        got = {"dpooled": self.region(10, self.N * 128, True).reshape(self.N, 128)}
        bt = self.region(8, 7 * 3 * 128, True).reshape(7, 3, 128)
        for i in range(7):
            got[f"bco{i}"] = bt[i, :, :dc.CO[i]]
            got[f"dW{i}"], got[f"dgamma{i}"], got[f"dbeta{i}"] = (b.read().double() for b in (self.gW[i], self.gG[i], self.gB[i]))
        got["dfcw"], got["dfcb"] = self.gfw.read().double().reshape(self.E, 128), self.gfb.read().double()
        return got

    def snapshot(self):
        torch.cuda.synchronize()
        return self.ws.clone(), [b.raw.clone() for b in [self.tokens, self.gfw, self.gfb] + self.gW + self.gG + self.gB + self.rm + self.rv]


G_AFTER = {0: ("g2", 12, 128), 1: ("g21", 13, 128), 2: ("g1", 14, 64), 3: ("g11", 12, 64), 4: ("g0", 13, 32)}


def _assert(ep, dt, cid, w, share_names=(), cap=lambda name: dc.SHARE_CAP):
    bad = []
    for name, r in w.rec.items():
        if r["index"] < 0:
            continue
        key = (ep, dt, re.sub(r"\d+$", "", name))
        if r["ratio"] >= _WORST.get(key, (-1,))[0]:
            _WORST[key] = (r["ratio"], r["share"], cid)
        if not r["finite"] or r["ratio"] > 1.0:
            bad.append(f"{name}: error {r['err']:.3e} is {r['ratio']:.3f} of its bar {r['bar']:.3e} at flat index {r['index']}")
        if name in share_names and r["share"] > cap(name):
            bad.append(f"{name}: {r['share']:.4f} of the elements have a boundary-dominated bar (cap {cap(name):.4f})")
    print(f"[deepresnet] {ep} {dt} {cid}: " + ", ".join(f"{k} {r['ratio']:.3f}" for k, r in w.rec.items() if r["index"] >= 0))
    assert not bad, f"{ep} {dt} {cid}:\n" + "\n".join(bad)


def _cap(c):
    return lambda name: dc.share_cap(c, name)


def _loss(dt, c, w, gf, gb):
    """measured loss of the E[x^2] - mean^2 statistics and the un-centred dgamma, in fp32 roundings (2^-24 relative)"""
    for i in range(7):
        ref, got = w.ref[f"fco{i}"], gf[f"fco{i}"]
        ex2 = ref[0] ** 2 + 1 / ref[1] ** 2
        rel = ((got[1] - ref[1]).abs() / ref[1]) / dc.U32
        k = int(rel.argmax())
        var = 1 / ref[1][k] ** 2 - dc.EPS
        dg_ref, dg = w.ref[f"dgamma{i}"], gb[f"dgamma{i}"]
        dgl = ((dg - dg_ref).abs() / dg_ref.abs().clamp_min(1e-30))[dg_ref.abs() > 0]
        print(f"[deepresnet-loss] {dt} {c['id']} bn{i}: worst rstd error {float(rel[k]):.2f} roundings (channel {k}: var {float(var):.3e}, "
              f"E[x^2]/var {float(ex2[k] / var.clamp_min(1e-30)):.3e}), implied var error {2 * float(rel[k]) * float((var + dc.EPS) / var.clamp_min(1e-30)):.2f} "
              f"roundings; worst dgamma error {float(dgl.max() / dc.U32) if dgl.numel() else 0:.2f} roundings")


def run_case(dt, c):
    """staged forward + backward (every stage observable), single-call forward + backward, inference"""
    N, P, E = c["N"], c["P"], c["E"]
    pr = Problem(dt, c)
    # ---- staged ----
    for st in range(6):
        pr.fwd(stage=st)
    gf = pr.got_forward()
    gs = {}
    for st in range(6):
        pr.bwd(stage=st)
        if st in G_AFTER:
            name, k, C = G_AFTER[st]
            gs[name] = pr.region(k, N * P * P * C).reshape(-1, C).clone()
    gb = pr.got_backward()
    w = dc.Walk(dt, {**gf, **gs, **gb})
    fw = dc.walk_forward(w, pr.prm, pr.x64, N, P, E, dc.EPS, pr.momentum, pr.running)
    dc.walk_backward(w, pr.prm, pr.x64, pr.dtok64, fw, N, P, E)
    _assert("staged", dt, c["id"], w, dc.SHARE_NAMES, _cap(c))
    if c["x"] in ("counts", "dc"):
        _loss(dt, c, w, gf, gb)
    # ---- single call ----
    pr.fresh()
    pr.fwd()
    gf = pr.got_forward()
    pr.bwd()
    gb = pr.got_backward()
    R = N * P * P
    gs = {"g11": pr.region(12, R * 64).reshape(-1, 64), "g0": pr.region(13, R * 32).reshape(-1, 32), "g1": pr.region(14, R * 64).reshape(-1, 64)}
    w = dc.Walk(dt, {**gf, **gs, **gb}, regen=("g2", "g21"))
    fw = dc.walk_forward(w, pr.prm, pr.x64, N, P, E, dc.EPS, pr.momentum, pr.running)
    dc.walk_backward(w, pr.prm, pr.x64, pr.dtok64, fw, N, P, E)
    _assert("single", dt, c["id"], w)
    # ---- inference on the running statistics ----
    pr.fresh(pass_running=True)            # (inference requires them, and must leave them untouched)
    pr.fwd(infer=True)
    w = dc.Walk(dt, pr.got_forward(infer=True))
    dc.walk_forward(w, pr.prm, pr.x64, N, P, E, dc.EPS, infer=True)
    _assert("infer", dt, c["id"], w, tuple(f"y{i}" for i in range(1, 7)), _cap(c))


def _params(cases):
    return [pytest.param(dt, c, id=f"{dt}-{c['id']}") for c in cases for dt in dc.case_dts(c)]


@gpu
@pytest.mark.parametrize("dt,c", _params(dc.CASES))
def test_train_and_infer_every_launch_against_fp64(dt, c):
    t0 = time.time()
    run_case(dt, c)
    torch.cuda.synchronize()
    _TIMES[f"{dt}-{c['id']}"] = time.time() - t0


# ---- fused inference kernel ---------------------------------------------------------------------------------------------
def _eval_cases():
    return [pytest.param(dt, P, N, id=f"{dt}-P{P}-N{N}") for dt, P, N in dc.eval_cases()]


@gpu
@pytest.mark.parametrize("dt,P,N", _eval_cases())
def test_fused_inference_tokens_against_fp64(dt, P, N):
    """the test folds BatchNorm in fp64 and rounds the folded weights to T itself ([c_out][tap][c_in]): the kernel alone"""
    N_ = _N()
    E = (1, 16, 64, 130)[(P + N) % 4]
    assert bool(N_.lib.mivit_deepresnet_eval_supported(dc.CODE[dt], P))
    p32 = dc.make_params(40 + P, E)
    x = dc.make_frames("rand", N, P, 3 + P)
    pk = dc.fold64(dc.to64(p32), dt)
    tdt = dc.DT[dt]
    dev = {k: (v.to(tdt) if k in ("w11", "w12", "w1s", "w21", "w22", "w2s") else v.float()).contiguous().cuda() for k, v in pk.items()}
    xb = torch.full((N * P * P + 2 * GUARD,), float("nan"))
    xb[GUARD:GUARD + N * P * P] = x.reshape(-1)
    xb = xb.cuda()
    tok = Guarded(N * E)
    order = ("w0", "b0", "w11", "w12", "w1s", "w21", "w22", "w2s", "b11", "b12", "b21", "b22", "wfc", "bfc")
    N_.check(N_.lib.mivit_deepresnet_eval_fwd(dc.CODE[dt], xb.data_ptr() + GUARD * 4, N, P, E, *[dev[k].data_ptr() for k in order],
                                              tok.ptr, _st()), "deepresnet_eval_fwd")
    torch.cuda.synchronize()
    got = tok.read().double().reshape(N, E)
    v = dc.eval_tokens(dt, {k: t.cuda() for k, t in pk.items()}, x.double().cuda(), N, P)
    w = dc.Walk(dt, {"tokens": got})
    w.out("tokens", v, "f32")
    _assert("eval_fwd", dt, f"P{P}-N{N}", w)


# ---- calling discipline ---------------------------------------------------------------------------------------------------
def _graph_stats():
    r, c, f = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    _N().lib.mivit_graph_stats(ctypes.byref(r), ctypes.byref(c), ctypes.byref(f))
    return r.value, c.value, f.value


@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_plain_capture_replay_are_bitwise_identical(dt):
    """the same call three times with identical arguments below the graph threshold: plain, capture, replay.  momentum 1:
    the running statistics the call rewrites do not depend on their previous value"""
    c = dict(next(c for c in dc.CASES if c["id"] == "whole-9x9-ragged"), momentum=1.0)
    assert dc.launch_plan(dt, c["N"], c["P"])["graph"]
    pr = Problem(dt, c)
    r0, c0, f0 = _graph_stats()
    snaps = []
    for _ in range(3):
        pr.fwd()
        snaps.append(pr.snapshot())
    r1, c1, f1 = _graph_stats()
    assert f1 == f0 and c1 == c0 + 1 and r1 >= r0 + 1, ((r0, c0, f0), (r1, c1, f1))
    for _ in range(3):
        pr.bwd()
        snaps.append(pr.snapshot())
    r2, c2, f2 = _graph_stats()
    assert f2 == f0 and c2 == c1 + 1 and r2 >= r1 + 1, ((r1, c1, f1), (r2, c2, f2))
    for base in (0, 3):
        for ws, bufs in snaps[base + 1:base + 3]:
            assert torch.equal(ws, snaps[base][0]), "workspace differs between plain / capture / replay"
            assert all(torch.equal(a, b) for a, b in zip(bufs, snaps[base][1]))
    pr.check_guard()


def _child():
    """one run of the three-case subset in this process (the environment switches are read once per process)"""
    for cid in dc.SUBSET:
        c = next(c for c in dc.CASES if c["id"] == cid)
        for dt in dc.case_dts(c):
            run_case(dt, c)
    torch.cuda.synchronize()
    print("[deepresnet] child OK")


@gpu
@pytest.mark.parametrize("var,val", [("MIVIT_DRN_NTW", "2"), ("MIVIT_DRN_SKIP_HALF", "0")])
def test_environment_switch_in_a_fresh_process(var, val):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, **{var: val})
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "[deepresnet] child OK" in r.stdout, f"{var}={val}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
