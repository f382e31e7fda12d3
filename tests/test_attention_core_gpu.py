"""The attention core (csrc/attention_fast.hip, csrc/attention.hip) against an fp64 reference that rounds what the kernels round.

`attn_ref` is softmax(q k^T * scale) v and its backward in fp64, on q, k, v, dO that already hold element-type values.  It rounds
the intermediates the kernels round, and only those (read off the kernels):
  * fast path (attention_fast.hip, bf16 and fp16 builds).  Forward: scores, softmax and P in fp32; `pack_frag` rounds P to the
    element type before P V.  Backward (`attn_bwd_fast2`): `pack4` rounds P before P^T dO; dS = scale * P * (dP - delta) is
    formed in fp32 and rounded by `pack4` before dS^T Q and (through the wave-private Simg image) before dS K; delta = sum P dP
    is taken on the UNROUNDED fp32 P.
  * general 16-bit kernels (attention.hip, T = bf16 / f16).  The P image (`Ps` forward, `Pa` backward) and the dS images
    (`dSn`, `dSt`) hold from_f32<T> of the fp32 values: the same two roundings, delta again on the fp32 P.
  * fp32 general kernels: the P / dS images are fp32, nothing is rounded.
Every path rounds its outputs once.  Errors are normalised per (batch, head) slice: max |got - ref| / max |ref| over the slice.
Bars (derived: one output rounding plus an occasional 1-ulp flip of a rounded P / dS element, with margin): bf16 1e-2,
fp16 2e-3, fp32 2e-5, for ctx, dq, dk and dv alike.

On top: exact tests of the 16-bit kernels (one-hot and uniform softmax), the bench shapes against both a GPU fp32 reference
over all heads and the fp64 reference on a sample, placement (NaN-guarded buffers through the raw C-ABI), determinism and
batch independence, rejection of shapes the kernels do not hold, and one model-level run of the general 16-bit kernels.
The tests without the `gpu` mark check the reference, the dispatch coverage and the exact-test construction on the CPU.
"""
import ctypes
import math
import os
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
CODE = {"f32": 0, "bf16": 1, "f16": 2}           # _native F32, BF16, F16
BAR = {"bf16": 1e-2, "f16": 2e-3, "f32": 2e-5}
OUTS = ("ctx", "dq", "dk", "dv")
LDS_LIMIT = 160 * 1024

_WORST = {}     # (dtype, path) -> worst per-head error seen in this run (printed at module teardown)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (dt, path), (e, what) in sorted(_WORST.items()):
        print(f"[attention core] worst per-head error {dt:4s} {path:10s} {e:.3e}  ({what})")


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def kernel_scale(Dh):
    """1.0f / sqrtf((float)Dh), as both kernels form it"""
    return float(np.float32(1.0) / np.sqrt(np.float32(Dh)))


def rounder(dt):
    """rounding to the element type (None for fp32: the fp32 kernels round nothing)"""
    if dt == "f32":
        return None
    t = DT[dt]
    return lambda x: x.to(t).to(x.dtype)


def attn_ref(q, k, v, do, scale, rnd=None):
    """q, k, v, do: [N, S, Dh].  Returns ctx, dq, dk, dv in the dtype of the inputs (fp64 on the CPU for the reference, fp32 on
    the GPU for the all-heads check).  `rnd` rounds P before P V / P^T dO and dS before dS K / dS^T Q; delta = sum P dP uses
    the unrounded P."""
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    pr = rnd(p) if rnd else p
    ctx = pr @ v
    dp = do @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = scale * p * (dp - delta)
    dsr = rnd(ds) if rnd else ds
    return ctx, dsr @ k, dsr.transpose(-1, -2) @ q, pr.transpose(-1, -2) @ do


def split_qkv(qkv, H):
    """[B, S, 3E] (q | k | v per token, head h at columns h*Dh) -> three [B*H, S, Dh]"""
    B, S, E3 = qkv.shape
    Dh = E3 // 3 // H
    x = qkv.reshape(B, S, 3, H, Dh).permute(2, 0, 3, 1, 4).reshape(3, B * H, S, Dh)
    return x[0], x[1], x[2]


def heads(t, H):
    """[B, S, E] -> [B*H, S, Dh]"""
    B, S, E = t.shape
    return t.reshape(B, S, H, E // H).permute(0, 2, 1, 3).reshape(B * H, S, E // H)


def head_err(got, ref):
    """per-head max |got - ref| / max |ref|; a head whose reference is exactly zero must be exactly zero"""
    d = (got.double() - ref.double()).abs().amax(dim=(1, 2))
    m = ref.double().abs().amax(dim=(1, 2))
    zero = torch.zeros_like(d)
    return torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), zero))


def check_heads(dt, path, got, ref, what=""):
    """got / ref: dicts of [N, S, Dh] per output; every head of every output within BAR[dt]"""
    for o in OUTS:
        e = head_err(got[o], ref[o])
        i = int(torch.argmax(e))
        worst = float(e[i])
        key = (dt, path)
        if key not in _WORST or worst > _WORST[key][0]:
            _WORST[key] = (worst, f"{o} {what}")
        assert worst <= BAR[dt], f"{path} {dt} {what}: {o} of head {i} (of {e.numel()}) off by {worst:.3e} > {BAR[dt]:.0e}"


def ref64(qkv, do, H, dt):
    """fp64 CPU reference of a [B, S, 3E] / [B, S, E] problem, per head"""
    q, k, v = (t.double().cpu() for t in split_qkv(qkv, H))
    ctx, dq, dk, dv = attn_ref(q, k, v, heads(do, H).double().cpu(), kernel_scale(q.shape[-1]), rounder(dt))
    return dict(ctx=ctx, dq=dq, dk=dk, dv=dv)


def got_heads(ctx, dqkv, H):
    q, k, v = split_qkv(dqkv, H)
    return dict(ctx=heads(ctx, H), dq=q, dk=k, dv=v)


# ---------------------------------------------------------------------------------------------------------------------
# dispatch rules, restated
# ---------------------------------------------------------------------------------------------------------------------
def fast_supported(S, Dh):
    """attention_fast.hip::attention_fast_supported (16-bit element types only)"""
    return Dh in (16, 32, 64) and 1 <= S and (S + 15) // 16 <= 8


def general_dims(S, Dh, f32, backward=True):
    """attention.hip::make_dims -> (per-wave LDS bytes, two_pass)"""
    KS = 4 if f32 else 32
    Sp = (S + 15) // 16 * 16
    kr = max(KS, 16)
    Skp = (S + kr - 1) // kr * kr
    Dp = (Dh + KS - 1) // KS * KS
    D16 = (Dh + 15) // 16 * 16
    ldq, ldk = (max(Dp, D16) + 1, Skp + 1) if f32 else (Dp + 8, Skp + 8)
    nat, tr, ps = Sp * ldq, D16 * ldk, max(Sp, Skp) * ldk
    if backward:
        per = 4 * nat + (0 if f32 else 3 * tr) + (2 if f32 else 3) * ps
    else:
        per = 3 * nat + (0 if f32 else tr) + ps
    esz = 4 if f32 else 2
    two_pass = backward and f32 and per * esz > LDS_LIMIT
    if two_pass:
        per = 4 * nat + ps
    return (per + 7) // 8 * 8 * esz, two_pass


def max_seq(dt, Dh):
    """attention.hip::attention_max_seq"""
    best = 0
    for S in range(1, 129):
        if general_dims(S, Dh, dt == "f32")[0] <= LDS_LIMIT or (dt != "f32" and fast_supported(S, Dh)):
            best = S
    return best


def _fast_dispatch_cases():
    src = open(os.path.join(ROOT, "moleculardiffusion_mivit_amd", "csrc", "attention_fast.hip")).read()
    body = src[src.index("#define FAST_DISPATCH"):]
    body = body[:body.index("default:")]
    cases = re.findall(r"case (\d+): return FN<(\d+), (\d+)>", body)
    assert all(int(key) == 10 * int(nt) + int(nd) for key, nt, nd in cases)     # the switch key is NT * 10 + ND
    return {(int(nt), int(nd)) for _, nt, nd in cases}


FAST_TILES = [(NT, ND) for ND in (1, 2, 4) for NT in range(1, 9)]
FAST_CASES = [(dt, NT, ND, S) for dt in ("bf16", "f16") for NT, ND in FAST_TILES
              for S in ((16 * NT, 16 * NT - 3) if NT > 1 else (16, 1))]
GEN_DH = (6, 8, 24, 48)
GEN_CASES = [(dt, Dh, S) for dt in ("bf16", "f16", "f32") for Dh in GEN_DH
             for S in sorted({1, 17, 33, 61, max_seq(dt, Dh)})]
# fp32 around the two_pass backward threshold (S >= 113 for Dh <= 32, S >= 81 at Dh = 64) and at the fast-path head dims
GEN_CASES += [("f32", 32, 112), ("f32", 32, 113), ("f32", 64, 80), ("f32", 64, 81), ("f32", 64, max_seq("f32", 64)),
              ("f32", 16, 128)]


def test_dispatch_coverage():
    """the fast-path parametrisation hits every case of FAST_DISPATCH, the restated rule admits exactly those, and every
    general case really is outside the fast path"""
    switch = _fast_dispatch_cases()
    assert len(switch) == 24
    rule = {((S + 15) // 16, Dh // 16) for S in range(1, 200) for Dh in (8, 16, 24, 32, 48, 64, 96) if fast_supported(S, Dh)}
    assert rule == switch
    hit = {((S + 15) // 16, ND) for dt, NT, ND, S in FAST_CASES if fast_supported(S, 16 * ND)}
    assert hit == switch
    for dt in ("bf16", "f16"):
        assert {(NT, ND) for d, NT, ND, S in FAST_CASES if d == dt and S % 16} == switch        # ragged last tile
        assert {(NT, ND) for d, NT, ND, S in FAST_CASES if d == dt and S % 16 == 0} == switch   # full last tile
    for dt, Dh, S in GEN_CASES:
        assert dt == "f32" or not fast_supported(S, Dh)
        assert general_dims(S, Dh, dt == "f32")[0] <= LDS_LIMIT
    assert any(Dh % 4 for _, Dh, _ in GEN_CASES)                          # scalar staging branch of stage_head
    # two_pass (fp32 backward, one score image) starts where make_dims puts it, and the cases cross it
    assert min(S for S in range(1, 129) if general_dims(S, 32, True)[1]) == 113
    assert min(S for S in range(1, 129) if general_dims(S, 64, True)[1]) == 81
    for Dh in GEN_DH + (32, 64):
        tp = {general_dims(S, Dh, True)[1] for d, D, S in GEN_CASES if d == "f32" and D == Dh}
        assert tp == {False, True}, Dh


def test_reference_matches_autograd_without_rounding():
    """with rounding off, attn_ref is the plain formula's autograd in fp64"""
    g = torch.Generator().manual_seed(5)
    for S, Dh in ((1, 8), (17, 6), (33, 32), (61, 64)):
        q, k, v, do = (torch.randn(6, S, Dh, generator=g, dtype=torch.float64) for _ in range(4))
        sc = kernel_scale(Dh)
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = torch.softmax((qa @ ka.transpose(-1, -2)) * sc, dim=-1) @ va
        out.backward(do)
        ctx, dq, dk, dv = attn_ref(q, k, v, do, sc)
        for a, b in ((ctx, out.detach()), (dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_reference_rounding_is_visible():
    """the rounded reference differs from the unrounded one by about the element type's ulp: the bars below are not met by
    accident of a reference that rounds nothing"""
    g = torch.Generator().manual_seed(6)
    q, k, v, do = (torch.randn(4, 33, 32, generator=g, dtype=torch.float64).bfloat16().double() for _ in range(4))
    a = attn_ref(q, k, v, do, kernel_scale(32))
    b = attn_ref(q, k, v, do, kernel_scale(32), rounder("bf16"))
    for x, y in zip(a, b):
        e = float(head_err(y, x).max())
        assert 1e-4 < e < 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# exact-test construction
# ---------------------------------------------------------------------------------------------------------------------
def onehot_c(Dh):
    """smallest integer c with 2 c^2 / sqrt(Dh) >= 150"""
    c = 1
    while 2 * c * c / math.sqrt(Dh) < 150:
        c += 1
    return c


def onehot_problem(B, S, H, Dh, seed):
    """keys j = c * (+-1 binary code of j over the first nb = min(7, Dh) dims), small random integers elsewhere; queries
    i = c * code(pi(i)), zero elsewhere, pi random (queries may share a key).  The best score leads by 2 c^2 / sqrt(Dh) >= 150,
    so P is exactly one-hot in fp32.  v, dO: integers in [-1, 1].  Returns qkv, do (fp32, CPU) and pi [B*H, S]."""
    nb = min(7, Dh)
    assert S <= 2 ** nb
    c = onehot_c(Dh)
    g = torch.Generator().manual_seed(seed)
    E = H * Dh
    bits = (torch.arange(S).view(S, 1) >> torch.arange(nb).view(1, nb)) & 1
    code = (1 - 2 * bits).float() * c                                   # [S, nb]
    pi = torch.randint(0, S, (B * H, S), generator=g)
    k = torch.randint(-3, 4, (B * H, S, Dh), generator=g).float()
    k[:, :, :nb] = code
    q = torch.zeros(B * H, S, Dh)
    q[:, :, :nb] = code[pi]
    v = torch.randint(-1, 2, (B * H, S, Dh), generator=g).float()
    do = torch.randint(-1, 2, (B * H, S, Dh), generator=g).float()
    s = (q.double() @ k.double().transpose(-1, -2)) * kernel_scale(Dh)
    top2 = s.topk(2, dim=-1).values
    assert torch.equal(s.argmax(-1), pi)
    assert float((top2[..., 0] - top2[..., 1]).min()) >= 150.0
    to_bshe = lambda t: t.reshape(B, H, S, Dh).permute(0, 2, 1, 3).reshape(B, S, E)     # noqa: E731
    qkv = torch.cat([to_bshe(q), to_bshe(k), to_bshe(v)], dim=-1)
    return qkv, to_bshe(do), pi


ONEHOT_CASES = [(dt, Dh, NT) for dt in ("bf16", "f16") for Dh in (16, 32, 64, 8) for NT in range(1, 9)]


def _onehot_S(NT):
    return 16 * NT if NT % 2 == 0 else 16 * NT - 5


def test_onehot_construction():
    """the margin holds at every case the GPU test runs, with values every element type represents"""
    assert [onehot_c(Dh) for Dh in (8, 16, 32, 64)] == [15, 18, 21, 25]
    for dt, Dh, NT in ONEHOT_CASES:
        if dt != "bf16":
            continue
        S = _onehot_S(NT)
        qkv, do, _ = onehot_problem(1, S, 2, Dh, _seed(Dh, NT))
        assert torch.equal(qkv.bfloat16().float(), qkv) and torch.equal(qkv.half().float(), qkv)
        assert Dh in (16, 32, 64) or S <= max_seq(dt, Dh)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every dispatch target against the fp64 reference (small B: B * H = 6 waves, a ragged last workgroup)
# ---------------------------------------------------------------------------------------------------------------------
def _run_ops(qkv, do, H):
    from moleculardiffusion_mivit_amd import ops
    x = qkv.detach().clone().requires_grad_(True)
    out = ops.attention(x, H)
    out.backward(do)
    torch.cuda.synchronize()
    return out.detach(), x.grad.detach()


def _randn_problem(dt, B, S, H, Dh, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3 * H * Dh, generator=g).to(DT[dt])
    do = torch.randn(B, S, H * Dh, generator=g).to(DT[dt])
    return qkv, do


def _against_fp64(dt, path, B, S, H, Dh):
    qkv, do = _randn_problem(dt, B, S, H, Dh, _seed(dt, B, S, H, Dh))
    ctx, dqkv = _run_ops(qkv.cuda(), do.cuda(), H)
    check_heads(dt, path, got_heads(ctx.cpu(), dqkv.cpu(), H), ref64(qkv, do, H, dt), f"B={B} S={S} H={H} Dh={Dh}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt,NT,ND,S", FAST_CASES, ids=[f"{d}-NT{a}-ND{b}-S{s}" for d, a, b, s in FAST_CASES])
def test_fast_path_against_fp64(dt, NT, ND, S):
    assert (S + 15) // 16 == NT and fast_supported(S, 16 * ND)
    _against_fp64(dt, "fast", 3, S, 2, 16 * ND)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,Dh,S", GEN_CASES, ids=[f"{d}-Dh{h}-S{s}" for d, h, s in GEN_CASES])
def test_general_kernels_against_fp64(dt, Dh, S):
    from moleculardiffusion_mivit_amd import _native as N
    assert N.lib.mivit_attention_max_seq(CODE[dt], Dh) == max_seq(dt, Dh)
    _against_fp64(dt, "general" if dt != "f32" else "f32", 3, S, 2, Dh)


REJECT_CASES = [("bf16", 24, max_seq("bf16", 24) + 1, "bwd"), ("f16", 48, max_seq("f16", 48) + 1, "bwd"),
                ("f32", 48, max_seq("f32", 48) + 1, "bwd"), ("bf16", 8, max_seq("bf16", 8) + 1, "bwd"),
                ("bf16", 16, 129, "fwd"), ("bf16", 16, 129, "bwd"), ("f16", 8, 129, "fwd"), ("f16", 32, 129, "bwd"),
                ("f32", 6, 129, "fwd"), ("f32", 6, 129, "bwd"), ("f32", 64, 129, "bwd")]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,Dh,S,which", REJECT_CASES, ids=[f"{w}-{d}-Dh{h}-S{s}" for d, h, s, w in REJECT_CASES])
def test_rejects_what_does_not_fit(dt, Dh, S, which):
    """past max_seq (or S = 129) the C entries fail with a message before launching anything: the output stays untouched.
    (The buffers are sized for the requested S, so even a launch would stay inside them.)"""
    from moleculardiffusion_mivit_amd import _native as N
    H = 1
    qkv = torch.zeros(1, S, 3 * H * Dh, dtype=DT[dt], device="cuda")
    out = torch.full((1, S, (3 if which == "bwd" else 1) * H * Dh), float("nan"), dtype=DT[dt], device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if which == "fwd":
        rc = N.lib.mivit_attention_fwd(CODE[dt], p(qkv), 1, S, H, Dh, p(out), st)
    else:
        dctx = torch.zeros(1, S, H * Dh, dtype=DT[dt], device="cuda")
        rc = N.lib.mivit_attention_bwd(CODE[dt], p(qkv), p(dctx), 1, S, H, Dh, p(out), st)
    torch.cuda.synchronize()
    assert rc != 0
    msg = N.lib.mivit_last_error().decode()
    assert re.search(r"does not fit|not supported", msg), msg
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: exact tests of the 16-bit kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt,Dh,NT", ONEHOT_CASES, ids=[f"{d}-Dh{h}-NT{n}" for d, h, n in ONEHOT_CASES])
def test_onehot_softmax_exact(dt, Dh, NT):
    """P exactly one-hot with a random key per query: ctx_i = v_pi(i) and dv_j = sum_{pi(i)=j} dO_i bitwise, dq = dk = 0
    (dS = P (dP - delta) vanishes on a one-hot row).  A permuted key / query, a wrong half-row exchange or a dropped /
    doubled token tile is an exact mismatch."""
    B, H, S = 2, 2, _onehot_S(NT)
    qkv, do, pi = onehot_problem(B, S, H, Dh, _seed(dt, Dh, NT))
    ctx, dqkv = _run_ops(qkv.to(DT[dt]).cuda(), do.to(DT[dt]).cuda(), H)
    got = {o: t.float().cpu() for o, t in got_heads(ctx, dqkv, H).items()}
    v = split_qkv(qkv, H)[2]
    dOh = heads(do, H)
    exp_ctx = torch.stack([v[n][pi[n]] for n in range(B * H)])
    exp_dv = torch.zeros_like(v)
    for n in range(B * H):
        exp_dv[n].index_add_(0, pi[n], dOh[n])
    assert torch.equal(got["ctx"], exp_ctx), "ctx"
    assert torch.equal(got["dv"], exp_dv), "dv"
    assert not bool(got["dq"].any()), "dq"
    assert not bool(got["dk"].any()), "dk"


UNIFORM_CASES = [(dt, Dh, S) for dt in ("bf16", "f16") for Dh in (16, 32, 64, 8) for S in (16, 32, 64, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,Dh,S", UNIFORM_CASES, ids=[f"{d}-Dh{h}-S{s}" for d, h, s in UNIFORM_CASES])
def test_uniform_softmax_exact(dt, Dh, S):
    """q = 0: P = 1/S exactly.  ctx = mean of v over keys and dv = mean of dO over queries bitwise, dk = dS^T q = 0 exactly;
    dq against the fp64 reference"""
    B, H = 2, 2
    g = torch.Generator().manual_seed(_seed("uniform", dt, Dh, S))
    E = H * Dh
    qkv = torch.randint(-1, 2, (B, S, 3 * E), generator=g).float()
    qkv[..., :E] = 0
    do = torch.randint(-1, 2, (B, S, E), generator=g).float()
    ctx, dqkv = _run_ops(qkv.to(DT[dt]).cuda(), do.to(DT[dt]).cuda(), H)
    got = {o: t.cpu() for o, t in got_heads(ctx, dqkv, H).items()}
    v = split_qkv(qkv, H)[2].double()
    mean_v = v.mean(dim=1, keepdim=True).expand_as(v)
    mean_do = heads(do, H).double().mean(dim=1, keepdim=True).expand_as(v)
    for t in (mean_v, mean_do):
        assert torch.equal(t.to(DT[dt]).double(), t)          # representable: the kernel's result must be exactly this
    assert torch.equal(got["ctx"].double(), mean_v), "ctx"
    assert torch.equal(got["dv"].double(), mean_do), "dv"
    assert not bool(got["dk"].any()), "dk"
    ref = ref64(qkv.to(DT[dt]), do.to(DT[dt]), H, dt)
    e = float(head_err(got["dq"], ref["dq"]).max())
    assert e <= BAR[dt], e


# ---------------------------------------------------------------------------------------------------------------------
# GPU: bench scale, placement, determinism, batch independence
# ---------------------------------------------------------------------------------------------------------------------
def sample_heads(n, k=256):
    """first 16, last 16 (the ragged last workgroup), the rest spread evenly"""
    if n <= k:
        return list(range(n))
    mid = np.linspace(16, n - 17, k - 32).round().astype(np.int64).tolist()
    return sorted(set(range(16)) | set(range(n - 16, n)) | set(mid))


BENCH_SHAPES = [("bf16", 16384, 33, 4, 32), ("bf16", 4096, 31, 4, 16), ("bf16", 4096, 61, 4, 16),
                ("f16", 4096, 31, 4, 16), ("f16", 4096, 61, 4, 16), ("bf16", 5461, 33, 3, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,B,S,H,Dh", BENCH_SHAPES, ids=[f"{d}-B{b}-S{s}-H{h}-Dh{e}" for d, b, s, h, e in BENCH_SHAPES])
def test_bench_scale(dt, B, S, H, Dh):
    """all heads against plain torch fp32 on the GPU (an independent code path, rounding P and dS like the kernel), a sample
    of heads against the fp64 CPU reference; bitwise repeatable; the last 70 sequences on their own give the same rows"""
    g = torch.Generator(device="cuda").manual_seed(_seed(dt, B, S, H, Dh))
    E = H * Dh
    qkv = torch.randn(B, S, 3 * E, generator=g, device="cuda").to(DT[dt])
    do = torch.randn(B, S, E, generator=g, device="cuda").to(DT[dt])
    ctx, dqkv = _run_ops(qkv, do, H)
    got = got_heads(ctx, dqkv, H)
    where = f"B={B} S={S} H={H} Dh={Dh}"
    # every head: GPU fp32
    with torch.no_grad():
        q, k, v = split_qkv(qkv.float(), H)
        r = attn_ref(q, k, v, heads(do.float(), H), kernel_scale(Dh), rounder(dt))
        check_heads(dt, "bench/fp32", got, dict(zip(OUTS, r)), where + " vs GPU fp32")
        del q, k, v, r
    # sampled heads: fp64 CPU
    idx = torch.tensor(sample_heads(B * H), device="cuda")
    q, k, v = (t[idx].double().cpu() for t in split_qkv(qkv, H))
    r = attn_ref(q, k, v, heads(do, H)[idx].double().cpu(), kernel_scale(Dh), rounder(dt))
    check_heads(dt, "bench/fp64", {o: t[idx].cpu() for o, t in got.items()}, dict(zip(OUTS, r)), where + " vs fp64")
    # one wave per (batch, head), no cross-wave reduction: bitwise
    ctx2, dqkv2 = _run_ops(qkv, do, H)
    assert torch.equal(ctx2, ctx) and torch.equal(dqkv2, dqkv), "not repeatable"
    ctx3, dqkv3 = _run_ops(qkv[B - 70:].contiguous(), do[B - 70:].contiguous(), H)
    assert torch.equal(ctx3, ctx[B - 70:]) and torch.equal(dqkv3, dqkv[B - 70:]), "depends on the rest of the batch"


PLACE_CASES = [("bf16", 33, 32), ("f16", 61, 16), ("bf16", 17, 64), ("f16", 128, 16), ("bf16", 33, 24), ("f16", 61, 6),
               ("f32", 113, 8), ("f32", 33, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,S,Dh", PLACE_CASES, ids=[f"{d}-S{s}-Dh{h}" for d, s, h in PLACE_CASES])
def test_placement_nan_guards(dt, S, Dh):
    """inputs between NaN guards, outputs inside NaN-filled buffers with guards on both sides, through the raw C-ABI:
    no NaN left in an output (every element written, no padding read), guards bitwise unchanged (nothing written outside),
    outputs bitwise equal to a plain call"""
    from moleculardiffusion_mivit_amd import _native as N
    B, H = 5, 3
    E, G = H * Dh, 256               # guard elements (a multiple of 16 bytes for every element type)
    t = DT[dt]
    qkv, do = _randn_problem(dt, B, S, H, Dh, _seed("place", dt, S, Dh))
    qkv, do = qkv.cuda(), do.cuda()
    ctx_ref, dqkv_ref = _run_ops(qkv, do, H)
    ibits = torch.int32 if dt == "f32" else torch.int16

    def guarded(src_or_n):
        n = src_or_n if isinstance(src_or_n, int) else src_or_n.numel()
        buf = torch.full((G + n + G,), float("nan"), dtype=t, device="cuda")
        if not isinstance(src_or_n, int):
            buf[G:G + n] = src_or_n.reshape(-1)
        return buf, buf.view(ibits).clone()

    def ptr(buf):
        return ctypes.c_void_p(buf.data_ptr() + G * buf.element_size())

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    qb, qb0 = guarded(qkv)
    ob, ob0 = guarded(do)
    cb, cb0 = guarded(B * S * E)
    gb, gb0 = guarded(B * S * 3 * E)
    N.check(N.lib.mivit_attention_fwd(CODE[dt], ptr(qb), B, S, H, Dh, ptr(cb), st), "attention_fwd")
    N.check(N.lib.mivit_attention_bwd(CODE[dt], ptr(qb), ptr(ob), B, S, H, Dh, ptr(gb), st), "attention_bwd")
    torch.cuda.synchronize()
    for name, buf, bits0 in (("qkv", qb, qb0), ("dctx", ob, ob0), ("ctx", cb, cb0), ("dqkv", gb, gb0)):
        b = buf.view(ibits)
        assert torch.equal(b[:G], bits0[:G]) and torch.equal(b[-G:], bits0[-G:]), f"{name}: guard overwritten"
    assert torch.equal(qb.view(ibits), qb0) and torch.equal(ob.view(ibits), ob0), "an input was written"
    ctx, dqkv = cb[G:-G], gb[G:-G]
    assert not bool(torch.isnan(ctx).any()), "ctx: element not written (or NaN read)"
    assert not bool(torch.isnan(dqkv).any()), "dqkv: element not written (or NaN read)"
    assert torch.equal(ctx.view(ibits), ctx_ref.reshape(-1).view(ibits))
    assert torch.equal(dqkv.view(ibits), dqkv_ref.reshape(-1).view(ibits))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one model through the general 16-bit kernels
# ---------------------------------------------------------------------------------------------------------------------
def _step(m, x, y):
    for p in m.parameters():
        p.grad = None
    out = m(x)
    loss = F.mse_loss(out, y)
    loss.backward()
    return out.detach(), float(loss.detach()), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("E,H", [(64, 8), (96, 4)], ids=["E64-H8", "E96-H4"])
def test_model_general_head_dim_bf16_against_fp32_parity_mode(E, H):
    """head dims 8 and 24 are outside the fast path and the fused layer blocks: the engine runs these layers per operator and
    the attention core through the general bf16 kernels.  Bands = those of
    test_bench_scale_gpu.py::test_c1_bf16_at_bench_batch_against_fp32_parity_mode."""
    from oracle import mivit_oracle as orc
    from util import build_product_model, rel_err
    from moleculardiffusion_mivit_amd import _native as N
    cfg = orc.MiViTConfig(embedding="linear", patch_size=16, embed_dim=E, num_heads=H, hidden_dim=2 * E, num_layers=2)
    S = 33
    assert not fast_supported(S, E // H)
    for fused in (N.lib.mivit_fused_layer_supported, N.lib.mivit_fused_layer_supported_w64):
        assert fused(CODE["bf16"], E, 2 * E, H, S) == 0
    x, y, _ = orc.closed_form_batch(256, S - 1, 16)
    x, y = x.cuda(), y.cuda()
    params = orc.closed_form_params(cfg)
    o32, l32, g32 = _step(build_product_model(cfg, "fp32", params), x, y)
    o16, l16, g16 = _step(build_product_model(cfg, "bf16", params), x, y)
    assert rel_err(o16, o32) < 5e-2
    assert abs(l16 - l32) <= 2e-2 * abs(l32)
    gscale = max(float(g.norm()) for g in g32.values())
    for k in g32:
        e = float((g16[k] - g32[k]).norm() / (g32[k].norm() + 1e-3 * gscale))
        assert e < 8e-2, (k, e)
