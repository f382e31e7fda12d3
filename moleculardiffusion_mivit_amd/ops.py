"""Operator-level autograd wrappers over the C-ABI kernels (include/mivit_hip.h, "Operator level").

Each function mirrors one torch op of the reference path (nn.Linear(+activation), nn.LayerNorm, the attention
core of MultiHeadAttention) and differentiates through the matching hand-written backward kernels.  Tensors must
be on the GPU; x may be float32 (fp32 MFMA), bfloat16 (bf16 MFMA, the fast path) or float16 (fp16 MFMA, general
kernels); weights / LayerNorm parameters are fp32.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return N.F32
    if t.dtype == torch.bfloat16:
        return N.BF16
    if t.dtype == torch.float16:
        return N.F16
    raise TypeError(f"unsupported dtype {t.dtype} (float32, bfloat16 or float16)")


def _gpu(*ts):
    for t in ts:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("MiViT HIP operators need GPU tensors (no CPU fallback exists in this package)")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, act):
        _gpu(x, W, b)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        W = W.contiguous().float()
        bb = b.contiguous().float() if b is not None else None
        M, K = x2.shape
        Nn = W.shape[0]
        y = torch.empty(M, Nn, dtype=x2.dtype, device=x2.device)
        pre = torch.empty_like(y) if act == N.ACT_GELU else None
        N.check(N.lib.mivit_linear_fwd(_dt(x2), _p(x2), 0, K, _p(W), _p(bb), M, Nn, K, act, None, 0, _p(y), Nn,
                                       _p(pre), _s(x2)), "mivit_linear_fwd")
        ctx.save_for_backward(x2, W, pre if pre is not None else y)
        ctx.act, ctx.shp, ctx.has_b = act, shp, b is not None
        return y.reshape(*shp[:-1], Nn)

    @staticmethod
    def backward(ctx, dy):
        x2, W, saved = ctx.saved_tensors
        M, K = x2.shape
        Nn = W.shape[0]
        dy2 = dy.reshape(M, Nn).contiguous().to(x2.dtype)
        dt = _dt(x2)
        if ctx.act != N.ACT_NONE:   # fold act' into dy first: d(pre) = dy * act'(saved)
            # the dgrad kernel applies act' to ITS output; here act sits on the linear's output, so use a tiny
            # identity-dgrad trick-free path: elementwise in torch (glue) -- kept out of the fused engine path.
            if ctx.act == N.ACT_RELU:
                dy2 = dy2 * (saved > 0).to(dy2.dtype)
            elif ctx.act == N.ACT_LEAKY_RELU:
                dy2 = dy2 * torch.where(saved > 0, 1.0, 0.01).to(dy2.dtype)
            else:
                u = saved.float()
                cdf = 0.5 * (1 + torch.erf(u * 0.7071067811865476))
                pdf = torch.exp(-0.5 * u * u) * 0.3989422804014327
                dy2 = (dy2.float() * (cdf + u * pdf)).to(dy2.dtype)
            dy2 = dy2.contiguous()
        dx = torch.empty_like(x2)
        N.check(N.lib.mivit_linear_dgrad(dt, _p(dy2), Nn, _p(W), M, Nn, K, N.ACT_NONE, None, 0, None, 0, _p(dx), K,
                                         _s(x2)), "mivit_linear_dgrad")
        dW = torch.empty_like(W)
        db = torch.empty(Nn, dtype=torch.float32, device=W.device) if ctx.has_b else None
        wsb = N.lib.mivit_linear_wgrad_workspace_bytes(M, Nn, K)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=W.device)
        N.check(N.lib.mivit_linear_wgrad(dt, _p(dy2), Nn, _p(x2), 0, K, M, Nn, K, _p(dW), _p(db), 0, _p(ws), ws.numel(),
                                         _s(x2)), "mivit_linear_wgrad")
        return dx.reshape(ctx.shp), dW, db, None


def linear(x, W, b=None, act=N.ACT_NONE):
    """act(x @ W^T + b): nn.Linear (+ relu / leaky_relu / gelu)."""
    return _Linear.apply(x, W, b, act)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        _gpu(x, w, b)
        shp = x.shape
        E = shp[-1]
        x2 = x.reshape(-1, E).contiguous()
        w, b = w.contiguous().float(), b.contiguous().float()
        M = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(M, dtype=torch.float32, device=x2.device)
        rstd = torch.empty_like(mean)
        N.check(N.lib.mivit_layernorm_fwd(_dt(x2), _p(x2), E, _p(w), _p(b), M, E, _p(y), E, 0, 0, 0, None, _p(mean),
                                          _p(rstd), _s(x2)), "mivit_layernorm_fwd")
        ctx.save_for_backward(x2, w, mean, rstd)
        ctx.shp = shp
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, w, mean, rstd = ctx.saved_tensors
        M, E = x2.shape
        dy2 = dy.reshape(M, E).contiguous().to(x2.dtype)
        dx = torch.empty_like(x2)
        dg = torch.empty(E, dtype=torch.float32, device=x2.device)
        db = torch.empty_like(dg)
        wsb = N.lib.mivit_layernorm_bwd_workspace_bytes(M, E)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=x2.device)
        N.check(N.lib.mivit_layernorm_bwd(_dt(x2), _p(dy2), E, _p(x2), E, _p(w), _p(mean), _p(rstd), M, E, 0, 0, 0,
                                          _p(dx), E, _p(dg), _p(db), 0, _p(ws), ws.numel(), _s(x2)),
                "mivit_layernorm_bwd")
        return dx.reshape(ctx.shp), dg, db


def layer_norm(x, weight, bias):
    """nn.LayerNorm over the last dimension (eps 1e-5)."""
    return _LayerNorm.apply(x, weight, bias)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, H):
        _gpu(qkv)
        B, S, E3 = qkv.shape
        E = E3 // 3
        qkv = qkv.contiguous()
        out = torch.empty(B, S, E, dtype=qkv.dtype, device=qkv.device)
        N.check(N.lib.mivit_attention_fwd(_dt(qkv), _p(qkv), B, S, H, E // H, _p(out), _s(qkv)), "mivit_attention_fwd")
        ctx.save_for_backward(qkv)
        ctx.H = H
        return out

    @staticmethod
    def backward(ctx, dctx):
        (qkv,) = ctx.saved_tensors
        B, S, E3 = qkv.shape
        E = E3 // 3
        dctx = dctx.contiguous().to(qkv.dtype)
        dqkv = torch.empty_like(qkv)
        N.check(N.lib.mivit_attention_bwd(_dt(qkv), _p(qkv), _p(dctx), B, S, ctx.H, E // ctx.H, _p(dqkv), _s(qkv)),
                "mivit_attention_bwd")
        return dqkv, None


def attention(qkv, num_heads):
    """softmax(q k^T / sqrt(Dh)) v per head, heads merged.  qkv: [B, S, 3E] = [q | k | v] per token."""
    return _Attention.apply(qkv, num_heads)


def deepresnet_eval_supported(dtype: torch.dtype, patch_size: int) -> bool:
    return bool(N.lib.mivit_deepresnet_eval_supported(N.BF16 if dtype == torch.bfloat16 else N.F32, int(patch_size)))


def deepresnet_eval(x: torch.Tensor, pack: dict, embed_dim: int) -> torch.Tensor:
    """Inference-mode DeepResNetEmbedding (reference models.py:230-257) in one fused kernel.
    x [N,P,P] fp32 frames; ``pack`` = BN-folded weights from ``DeepResNetEmbedding.folded``; returns [N,E] fp32."""
    _gpu(x)
    x = x.contiguous().float()
    n, p, p2 = x.shape
    assert p == p2, "square frames expected"
    out = torch.empty(n, embed_dim, device=x.device, dtype=torch.float32)
    if n == 0:
        return out
    order = ("w0", "b0", "w11", "w12", "w1s", "w21", "w22", "w2s", "b11", "b12", "b21", "b22", "wfc", "bfc")
    N.check(N.lib.mivit_deepresnet_eval_fwd(_dt(pack["w11"]), _p(x), n, p, embed_dim, *[_p(pack[k]) for k in order],
                                            _p(out), _s(x)), "mivit_deepresnet_eval_fwd")
    return out


def deepresnet_train_supported(dtype: torch.dtype, patch_size: int) -> bool:
    return bool(N.lib.mivit_deepresnet_train_supported(N.BF16 if dtype == torch.bfloat16 else N.F32, int(patch_size)))


class _DeepResNetTrain(torch.autograd.Function):
    """Training-mode DeepResNetEmbedding (reference models.py:230-257) on the hand-written conv / BatchNorm kernels.
    Inputs after ``x``: for each of the 7 conv+BN pairs (weight, gamma, beta), then fc.weight, fc.bias  (23 tensors)."""

    @staticmethod
    def forward(ctx, x, dtype_code, momentum, eps, running, *params):
        n, p, _ = x.shape
        e = params[21].shape[0]
        prm = N.DeepResNetParams()
        for i in range(7):
            w, g, b = params[3 * i:3 * i + 3]
            rm, rv = running[i]
            prm.conv[i] = N.ConvBn(w.data_ptr(), g.data_ptr(), b.data_ptr(), rm.data_ptr() if rm is not None else None,
                                   rv.data_ptr() if rv is not None else None)
        prm.fc_weight, prm.fc_bias = params[21].data_ptr(), params[22].data_ptr()
        nbytes = N.lib.mivit_deepresnet_train_workspace_bytes(dtype_code, n, p, e)
        if nbytes == 0:
            raise N.MivitError(f"DeepResNet training kernels do not support frame side {p}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        tokens = torch.empty(n, e, device=x.device, dtype=torch.float32)
        N.check(N.lib.mivit_deepresnet_train_fwd(dtype_code, ctypes.addressof(prm), _p(x), n, p, e, momentum, eps, _p(tokens),
                                                 _p(ws), nbytes, _s(x)), "mivit_deepresnet_train_fwd")
        ctx.save_for_backward(x, ws, *params)
        ctx.meta = (dtype_code, n, p, e, eps, nbytes)
        return tokens

    @staticmethod
    def backward(ctx, dtokens):
        x, ws, *params = ctx.saved_tensors
        dtype_code, n, p, e, eps, nbytes = ctx.meta
        prm, gr = N.DeepResNetParams(), N.DeepResNetGrads()
        grads = [torch.empty_like(t) for t in params]
        for i in range(7):
            w, g, b = params[3 * i:3 * i + 3]
            prm.conv[i] = N.ConvBn(w.data_ptr(), g.data_ptr(), b.data_ptr(), None, None)
            gr.conv[i] = N.ConvBnGrad(*[t.data_ptr() for t in grads[3 * i:3 * i + 3]])
        prm.fc_weight, prm.fc_bias = params[21].data_ptr(), params[22].data_ptr()
        gr.fc_weight, gr.fc_bias = grads[21].data_ptr(), grads[22].data_ptr()
        dtokens = dtokens.contiguous().float()
        N.check(N.lib.mivit_deepresnet_train_bwd(dtype_code, ctypes.addressof(prm), _p(x), _p(dtokens), n, p, e, eps,
                                                 ctypes.addressof(gr), _p(ws), nbytes, _s(x)), "mivit_deepresnet_train_bwd")
        return (None, None, None, None, None, *grads)


DEEPRESNET_STAGES = 6


class _DeepResNetTrainSync(torch.autograd.Function):
    """_DeepResNetTrain with BatchNorm statistics synchronised over a process group: the native forward /
    backward run stage by stage with one small fp64 all-reduce of the BatchNorm sums between stages, so every rank
    normalises with the statistics of the whole minibatch -- what the single-device reference (models.py:206-225,233)
    computes.  d gamma / d beta stay per-rank sums like every other parameter gradient (the DP all-reduce averages them)."""

    @staticmethod
    def forward(ctx, x, dtype_code, momentum, eps, running, group, *params):
        import torch.distributed as dist
        n, p, _ = x.shape
        e = params[21].shape[0]
        prm = N.DeepResNetParams()
        for i in range(7):
            w, g, b = params[3 * i:3 * i + 3]
            rm, rv = running[i]
            prm.conv[i] = N.ConvBn(w.data_ptr(), g.data_ptr(), b.data_ptr(), rm.data_ptr() if rm is not None else None,
                                   rv.data_ptr() if rv is not None else None)
        prm.fc_weight, prm.fc_bias = params[21].data_ptr(), params[22].data_ptr()
        nbytes = N.lib.mivit_deepresnet_train_workspace_bytes(dtype_code, n, p, e)
        if nbytes == 0:
            raise N.MivitError(f"DeepResNet training kernels do not support frame side {p}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        tokens = torch.empty(n, e, device=x.device, dtype=torch.float32)
        count = torch.full((1,), float(n * p * p), dtype=torch.float64, device=x.device)
        dist.all_reduce(count, group=group)
        stats = torch.zeros(2, 3, 128, dtype=torch.float64, device=x.device)
        for stage in range(DEEPRESNET_STAGES):
            N.check(N.lib.mivit_deepresnet_train_fwd_stage(dtype_code, ctypes.addressof(prm), _p(x), n, p, e, momentum, eps,
                                                           _p(tokens), _p(ws), nbytes, stage, _p(count), _p(stats), _s(x)),
                    "mivit_deepresnet_train_fwd_stage")
            if stage + 1 < DEEPRESNET_STAGES:
                dist.all_reduce(stats, group=group)
        ctx.save_for_backward(x, ws, count, *params)
        ctx.meta = (dtype_code, n, p, e, eps, nbytes, group)
        return tokens

    @staticmethod
    def backward(ctx, dtokens):
        import torch.distributed as dist
        x, ws, count, *params = ctx.saved_tensors
        dtype_code, n, p, e, eps, nbytes, group = ctx.meta
        prm, gr = N.DeepResNetParams(), N.DeepResNetGrads()
        grads = [torch.empty_like(t) for t in params]
        for i in range(7):
            w, g, b = params[3 * i:3 * i + 3]
            prm.conv[i] = N.ConvBn(w.data_ptr(), g.data_ptr(), b.data_ptr(), None, None)
            gr.conv[i] = N.ConvBnGrad(*[t.data_ptr() for t in grads[3 * i:3 * i + 3]])
        prm.fc_weight, prm.fc_bias = params[21].data_ptr(), params[22].data_ptr()
        gr.fc_weight, gr.fc_bias = grads[21].data_ptr(), grads[22].data_ptr()
        dtokens = dtokens.contiguous().float()
        stats = torch.zeros(2, 3, 128, dtype=torch.float64, device=x.device)
        for stage in range(DEEPRESNET_STAGES):
            N.check(N.lib.mivit_deepresnet_train_bwd_stage(dtype_code, ctypes.addressof(prm), _p(x), _p(dtokens), n, p, e, eps,
                                                           ctypes.addressof(gr), _p(ws), nbytes, stage, _p(count), _p(stats),
                                                           _s(x)), "mivit_deepresnet_train_bwd_stage")
            if stage + 1 < DEEPRESNET_STAGES:
                dist.all_reduce(stats[0], group=group)       # stats[1] keeps this rank's sums (d gamma / d beta)
        return (None, None, None, None, None, None, *grads)


def deepresnet_train_sync(x, dtype, momentum, eps, running, params, group=None):
    """deepresnet_train with BatchNorm statistics taken over every rank of ``group`` (default process group)."""
    _gpu(x, *params)
    for t in params:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("DeepResNet parameters must be contiguous float32 tensors")
    return _DeepResNetTrainSync.apply(x.contiguous().float(), N.BF16 if dtype == torch.bfloat16 else N.F32, float(momentum),
                                      float(eps), running, group, *params)


def deepresnet_train(x, dtype, momentum, eps, running, params):
    """x [N,P,P] fp32 frames -> tokens [N,E] fp32; ``running`` = 7 pairs (running_mean, running_var) updated in place
    (or (None, None)); ``params`` = the 23 parameter tensors (fp32, contiguous, reference layouts)."""
    _gpu(x, *params)
    for t in params:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("DeepResNet parameters must be contiguous float32 tensors")
    return _DeepResNetTrain.apply(x.contiguous().float(), N.BF16 if dtype == torch.bfloat16 else N.F32, float(momentum),
                                  float(eps), running, *params)


@torch.no_grad()
def deepresnet_infer(x, dtype, eps, running, params, chunk_frames: int = 8192):
    """Inference-mode DeepResNetEmbedding on the layer-by-layer kernels (any frame side; running statistics).
    Frames are processed in chunks so the activation workspace stays bounded."""
    _gpu(x, *params)
    x = x.contiguous().float()
    n, p, _ = x.shape
    e = params[21].shape[0]
    code = N.BF16 if dtype == torch.bfloat16 else N.F32
    prm = N.DeepResNetParams()
    for i in range(7):
        w, g, b = params[3 * i:3 * i + 3]
        prm.conv[i] = N.ConvBn(w.data_ptr(), g.data_ptr(), b.data_ptr(), running[i][0].data_ptr(), running[i][1].data_ptr())
    prm.fc_weight, prm.fc_bias = params[21].data_ptr(), params[22].data_ptr()
    out = torch.empty(n, e, device=x.device, dtype=torch.float32)
    ws = None
    for f0 in range(0, n, chunk_frames):
        m = min(chunk_frames, n - f0)
        nbytes = N.lib.mivit_deepresnet_train_workspace_bytes(code, m, p, e)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        N.check(N.lib.mivit_deepresnet_infer(code, ctypes.addressof(prm), _p(x[f0:f0 + m]), m, p, e, float(eps), _p(out[f0:f0 + m]),
                                             _p(ws), ws.numel(), _s(x)), "mivit_deepresnet_infer")
    return out


# ---------------------------------------------------------------------------------------------------------------
# fused encoder-layer blocks (csrc/fused_fwd.hip / fused_bwd.hip), bf16 or fp16, 4 heads, E = 128 / F = 256 or E = 64 / F = 128
# ---------------------------------------------------------------------------------------------------------------
_FUSED_DTYPES = {torch.bfloat16: "", torch.float16: "_f16"}


def _fused_entry(name: str, embed_dim: int, hidden_dim=None, dtype=torch.bfloat16):
    """the C entry point of a fused block for this layer width and element type (the kernels are compiled per width and type:
    anything else is refused here, before a launch that would index past the tensors or read them as the wrong type)"""
    if embed_dim not in (64, 128) or (hidden_dim is not None and hidden_dim != 2 * embed_dim):
        raise ValueError(f"{name}: fused blocks exist for E=128/F=256 and E=64/F=128, got E={embed_dim}"
                         + (f" F={hidden_dim}" if hidden_dim is not None else ""))
    if dtype not in _FUSED_DTYPES:
        raise TypeError(f"{name}: fused blocks exist for bfloat16 and float16, got {dtype}")
    return getattr(N.lib, name + ("_w64" if embed_dim == 64 else "") + _FUSED_DTYPES[dtype])


def _same_dtype(name, *ts):
    """the element type of a fused block's 16-bit tensors (all of them must share it)"""
    dt = ts[0].dtype
    for t in ts:
        if t.dtype != dt:
            raise TypeError(f"{name}: 16-bit operands must share one dtype, got {dt} and {t.dtype}")
    return dt


def fused_layer_supported(embed_dim: int, hidden_dim: int, num_heads: int, tokens: int, dtype=torch.bfloat16) -> bool:
    if embed_dim not in (64, 128) or dtype not in _FUSED_DTYPES:
        return False
    code = N.BF16 if dtype == torch.bfloat16 else N.F16
    return bool(_fused_entry("mivit_fused_layer_supported", embed_dim, dtype=dtype)(code, embed_dim, hidden_dim, num_heads, tokens))


def _f32(t):
    return None if t is None else t.contiguous().float()


@torch.no_grad()
def attn_block_fwd(n_in, gamma_in, beta_in, Wqkv, bqkv, Wo, bo, gamma_out, beta_out, extras=False):
    """n_in [B,S,E] bf16 or fp16 (normalised tokens; x = gamma_in * n_in + beta_in, or n_in itself when gamma_in is None);
    Wqkv [3E,E] / Wo [E,E] of the same dtype; returns dict(n, rstd, ctx[, x, z, mean, qkv]) -- reference models.py:33-59,100-102."""
    _gpu(n_in, Wqkv, Wo)
    B, S, E = n_in.shape
    dt = _same_dtype("attn_block_fwd", n_in, Wqkv, Wo)
    entry = _fused_entry("mivit_attn_block_fwd", E, dtype=dt)
    n_in = n_in.contiguous()
    dev = n_in.device
    out = {"n": torch.empty(B, S, E, dtype=dt, device=dev), "rstd": torch.empty(B, S, device=dev),
           "ctx": torch.empty(B, S, E, dtype=dt, device=dev)}
    if extras:
        out.update(x=torch.empty_like(out["n"]), z=torch.empty_like(out["n"]), mean=torch.empty(B, S, device=dev),
                   qkv=torch.empty(B, S, 3 * E, dtype=dt, device=dev))
    gi, bi, go, bo_ = _f32(gamma_in), _f32(beta_in), _f32(gamma_out), _f32(beta_out)
    bq, bo2 = _f32(bqkv), _f32(bo)
    if tuple(Wqkv.shape) != (3 * E, E) or tuple(Wo.shape) != (E, E):
        raise ValueError(f"attn_block_fwd: weights {tuple(Wqkv.shape)}, {tuple(Wo.shape)} do not match E={E}")
    N.check(entry(_p(n_in), _p(gi), _p(bi), _p(Wqkv.contiguous()), _p(bq), _p(Wo.contiguous()), _p(bo2),
                  _p(go), _p(bo_), B, S, _p(out["ctx"]), _p(out["n"]), _p(out["rstd"]), _p(out.get("x")),
                  _p(out.get("z")), _p(out.get("mean")), _p(out.get("qkv")), _s(n_in)),
            "mivit_attn_block_fwd")
    return out


@torch.no_grad()
def mlp_block_fwd(n_in, gamma_in, beta_in, W1, b1, W2, b2, gamma_out, beta_out, act=N.ACT_RELU, extras=False):
    """n_in [M,E] bf16 or fp16; W1 [F,E], W2 [E,F] of the same dtype; returns dict(n, rstd[, x, z, mean, h, u]) --
    models.py:72-77,104-106."""
    _gpu(n_in, W1, W2)
    M, E = n_in.shape
    Fh = W1.shape[0]
    dt = _same_dtype("mlp_block_fwd", n_in, W1, W2)
    entry = _fused_entry("mivit_mlp_block_fwd", E, Fh, dtype=dt)
    n_in = n_in.contiguous()
    dev = n_in.device
    out = {"n": torch.empty(M, E, dtype=dt, device=dev), "rstd": torch.empty(M, device=dev)}
    if extras:
        out.update(x=torch.empty_like(out["n"]), z=torch.empty_like(out["n"]), mean=torch.empty(M, device=dev),
                   h=torch.empty(M, Fh, dtype=dt, device=dev), u=torch.empty(M, Fh, dtype=dt, device=dev))
    gi, bi, go, bo_ = _f32(gamma_in), _f32(beta_in), _f32(gamma_out), _f32(beta_out)
    b1f, b2f = _f32(b1), _f32(b2)
    if tuple(W1.shape) != (Fh, E) or tuple(W2.shape) != (E, Fh):
        raise ValueError(f"mlp_block_fwd: weights {tuple(W1.shape)}, {tuple(W2.shape)} do not match E={E}")
    N.check(entry(_p(n_in), _p(gi), _p(bi), _p(W1.contiguous()), _p(b1f), _p(W2.contiguous()), _p(b2f),
                  _p(go), _p(bo_), M, act, _p(out["n"]), _p(out["rstd"]), _p(out.get("x")), _p(out.get("z")),
                  _p(out.get("mean")), _p(out.get("h")), _p(out.get("u")), _s(n_in)), "mivit_mlp_block_fwd")
    return out


@torch.no_grad()
def mlp_block_bwd(dy, n2, rstd2, gamma2, n1, gamma1, beta1, W1, b1, W2, act=N.ACT_RELU):
    """Backward of the feed-forward block (see include/mivit_hip.h), dy / n2 / n1 / W1 / W2 all bf16 or all fp16:
    returns dict(dx1 [that dtype], dW1, db1, dW2, db2, dgamma2, dbeta2 [fp32])."""
    _gpu(dy, n2, n1, W1, W2)
    M, E = dy.shape
    Fh = W1.shape[0]
    dt = _same_dtype("mlp_block_bwd", dy, n2, n1, W1, W2)
    dev = dy.device
    out = {"dx1": torch.empty(M, E, dtype=dt, device=dev), "dW1": torch.empty(Fh, E, device=dev),
           "db1": torch.empty(Fh, device=dev), "dW2": torch.empty(E, Fh, device=dev), "db2": torch.empty(E, device=dev),
           "dgamma2": torch.empty(E, device=dev), "dbeta2": torch.empty(E, device=dev)}
    if tuple(W1.shape) != (Fh, E) or tuple(W2.shape) != (E, Fh):
        raise ValueError(f"mlp_block_bwd: weights {tuple(W1.shape)}, {tuple(W2.shape)} do not match E={E}")
    nbytes = _fused_entry("mivit_mlp_block_bwd_workspace_bytes", E, Fh, dtype=dt)(M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = [dy.contiguous(), n2.contiguous(), _f32(rstd2), _f32(gamma2), n1.contiguous(), _f32(gamma1), _f32(beta1), W1.contiguous(),
            _f32(b1), W2.contiguous()]
    N.check(_fused_entry("mivit_mlp_block_bwd", E, Fh, dtype=dt)(
                *[_p(t) for t in args], M, act, _p(out["dx1"]), _p(out["dW1"]), _p(out["db1"]), _p(out["dW2"]),
                _p(out["db2"]), _p(out["dgamma2"]), _p(out["dbeta2"]), _p(ws), nbytes, _s(dy)),
            "mivit_mlp_block_bwd")
    return out


@torch.no_grad()
def attn_out_bwd(dy, n1, rstd1, gamma1, ctx, Wo):
    """LayerNorm-1 backward + out-projection backward (include/mivit_hip.h), dy / n1 / ctx / Wo all bf16 or all fp16:
    dict(dz1, dctx [that dtype], dWo, dbo, dgamma1, dbeta1 [fp32])."""
    _gpu(dy, n1, ctx, Wo)
    M, E = dy.shape
    dt = _same_dtype("attn_out_bwd", dy, n1, ctx, Wo)
    dev = dy.device
    out = {"dz1": torch.empty(M, E, dtype=dt, device=dev), "dctx": torch.empty(M, E, dtype=dt, device=dev),
           "dWo": torch.empty(E, E, device=dev), "dbo": torch.empty(E, device=dev), "dgamma1": torch.empty(E, device=dev),
           "dbeta1": torch.empty(E, device=dev)}
    if tuple(Wo.shape) != (E, E):
        raise ValueError(f"attn_out_bwd: weight {tuple(Wo.shape)} does not match E={E}")
    nbytes = _fused_entry("mivit_attn_out_bwd_workspace_bytes", E, dtype=dt)(M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = [dy.contiguous(), n1.contiguous(), _f32(rstd1), _f32(gamma1), ctx.contiguous(), Wo.contiguous()]
    N.check(_fused_entry("mivit_attn_out_bwd", E, dtype=dt)(
                *[_p(t) for t in args], M, _p(out["dz1"]), _p(out["dctx"]), _p(out["dWo"]), _p(out["dbo"]),
                _p(out["dgamma1"]), _p(out["dbeta1"]), _p(ws), nbytes, _s(dy)), "mivit_attn_out_bwd")
    return out


@torch.no_grad()
def qkv_bwd(dqkv, x, Wqkv, res, fix_gamma=None, fix_beta=None):
    """q|k|v projection backward in one pass over dqkv (include/mivit_hip.h), dqkv / x / Wqkv / res all bf16 or all fp16:
    dict(dx, dW, db); dx = dqkv Wqkv + res.  With fix_gamma / fix_beta [E] the projection's input is fix_gamma * x + fix_beta
    (x a LayerNorm's normalised output): dW = (dqkv^T x) diag(fix_gamma) + db (x) fix_beta."""
    _gpu(dqkv, x, Wqkv, res)
    M, E = x.shape
    if tuple(dqkv.shape) != (M, 3 * E) or tuple(Wqkv.shape) != (3 * E, E) or tuple(res.shape) != (M, E):
        raise ValueError(f"qkv_bwd: shapes {tuple(dqkv.shape)}, {tuple(Wqkv.shape)}, {tuple(res.shape)} do not match x {tuple(x.shape)}")
    if (fix_gamma is None) != (fix_beta is None):
        raise ValueError("qkv_bwd: the input affine needs both fix_gamma and fix_beta")
    dt = _same_dtype("qkv_bwd", dqkv, x, Wqkv, res)
    dev = x.device
    out = {"dx": torch.empty(M, E, dtype=dt, device=dev), "dW": torch.empty(3 * E, E, device=dev),
           "db": torch.empty(3 * E, device=dev)}
    nbytes = _fused_entry("mivit_qkv_bwd_workspace_bytes", E, dtype=dt)(M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = [dqkv.contiguous(), x.contiguous(), Wqkv.contiguous(), res.contiguous()]
    if fix_gamma is None:
        N.check(_fused_entry("mivit_qkv_bwd", E, dtype=dt)(*[_p(t) for t in args], M, _p(out["dx"]), _p(out["dW"]), _p(out["db"]),
                                                           _p(ws), nbytes, _s(x)), "mivit_qkv_bwd")
    else:
        fg, fb = _f32(fix_gamma), _f32(fix_beta)
        N.check(_fused_entry("mivit_qkv_bwd_affine", E, dtype=dt)(*[_p(t) for t in args], M, _p(out["dx"]), _p(out["dW"]),
                                                                  _p(out["db"]), _p(fg), _p(fb), _p(ws), nbytes, _s(x)),
                "mivit_qkv_bwd_affine")
    return out


def trajectory_features(traj: torch.Tensor, nPosPerFrame: int = 1, dt: float = 1.0, return_average: bool = False):
    """The 25 descriptors of helpers/features.compute_diffusion_features for every trajectory of a GPU batch (csrc/features.hip):
    traj [N, T, 2] float32 / float64 sub-step positions -> features [N, 25] float64 (NaN where the reference gives NaN),
    frames of nPosPerFrame sub-steps averaged in the input precision first; with return_average also the averaged positions
    [N, T // nPosPerFrame, 2] in the input dtype."""
    _gpu(traj)
    if traj.dim() != 3 or traj.shape[-1] != 2:
        raise ValueError(f"trajectories must be [N, T, 2], got {tuple(traj.shape)}")
    if traj.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {traj.dtype} (float32 or float64)")
    traj = traj.contiguous()
    n, steps, _ = traj.shape
    nf = steps // nPosPerFrame if nPosPerFrame >= 1 else 0
    feats = torch.empty(n, 25, dtype=torch.float64, device=traj.device)
    avg = torch.empty(n, nf, 2, dtype=traj.dtype, device=traj.device) if return_average else None
    wsb = N.lib.mivit_trajectory_features_workspace_bytes(n, steps, nPosPerFrame)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=traj.device)
    N.check(N.lib.mivit_trajectory_features(_p(traj), N.F32 if traj.dtype == torch.float32 else N.F64, n, steps,
                                            nPosPerFrame, float(dt), _p(feats), _p(avg), _p(ws), ws.numel(), _s(traj)),
            "mivit_trajectory_features")
    return (feats, avg) if return_average else feats


def _frames_f32(x, name):
    _gpu(x)
    if x.dtype != torch.float32:
        raise TypeError(f"{name}: frames must be float32, got {x.dtype}")
    return x.contiguous()


def rl_tv_deconvolve(frames: torch.Tensor, psf, iterations_list, tv_weight: float = 0.01) -> torch.Tensor:
    """Richardson-Lucy + total-variation deconvolution of every frame (csrc/deconv.hip, mivit_rl_tv_deconvolve), the batched
    helpers/generation.richardson_lucy_tv_iter_list: frames [B, S, H, W] float32 on the GPU, psf [K, K] (any float dtype,
    used in float64), iterations_list strictly increasing 0-based iteration indices -> [B, len(iterations_list), S, H, W]
    float32, the estimate after each listed iteration (iterations_list[-1] + 1 iterations run)."""
    frames = _frames_f32(frames, "rl_tv_deconvolve")
    if frames.dim() != 4:
        raise ValueError(f"frames must be [B, S, H, W], got {tuple(frames.shape)}")
    psf = torch.as_tensor(psf).to(device=frames.device, dtype=torch.float64).contiguous()
    if psf.dim() != 2 or psf.shape[0] != psf.shape[1]:
        raise ValueError(f"psf must be square [K, K], got {tuple(psf.shape)}")
    snaps = [int(i) for i in iterations_list]
    B, S, H, W = frames.shape
    out = torch.empty(B, len(snaps), S, H, W, dtype=torch.float32, device=frames.device)
    arr = (ctypes.c_int * max(1, len(snaps)))(*snaps)
    N.check(N.lib.mivit_rl_tv_deconvolve(_p(frames), B, S, H, W, _p(psf), psf.shape[0], arr, len(snaps),
                                         float(tv_weight), _p(out), _s(frames)), "mivit_rl_tv_deconvolve")
    return out


def gaussian_filter_frames(frames: torch.Tensor, sigma: float, truncate: float = 4.0) -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(frame, sigma, mode='nearest', truncate) of every [H, W] frame of a float32 GPU tensor
    [..., H, W] (csrc/deconv.hip, mivit_gaussian_filter_frames; fp64 inside, float32 out)."""
    frames = _frames_f32(frames, "gaussian_filter_frames")
    if frames.dim() < 2:
        raise ValueError(f"frames must be [..., H, W], got {tuple(frames.shape)}")
    H, W = frames.shape[-2:]
    out = torch.empty_like(frames)
    N.check(N.lib.mivit_gaussian_filter_frames(_p(frames), frames.numel() // max(1, H * W), H, W, float(sigma),
                                               float(truncate), _p(out), _s(frames)), "mivit_gaussian_filter_frames")
    return out


DOG_PEAKS_MAX_RADIUS, DOG_PEAKS_MAX_CAPACITY = 16, 2048


def dog_peaks(movie: torch.Tensor, w1, w2, threshold_percentage: float = 0.1, min_distance: int = 3,
              max_peaks_per_frame: int = 512, return_dog: bool = True):
    """Difference-of-Gaussians particle detection of a whole movie (csrc/tracking.hip, mivit_dog_peaks): movie [F, H, W]
    float32 on the GPU; w1 / w2 the half kernels (w[0] centre, w[k] weight at distance k, float64) of the narrow and the wide
    Gaussian, as helpers/tracking.gaussian_half_kernel builds them -> (count [F] int32, coords [F, cap, 2] int32 (y, x),
    values [F, cap] float32, dog [F, H, W] float32 or None).  Peaks of a frame are ordered by value descending, ties by
    row-major index.  Raises if a frame has more candidates than max_peaks_per_frame: nothing is truncated silently."""
    movie = _frames_f32(movie, "dog_peaks")
    if movie.dim() != 3:
        raise ValueError(f"movie must be [F, H, W], got {tuple(movie.shape)}")
    import numpy as np
    w1 = np.ascontiguousarray(w1, dtype=np.float64)
    w2 = np.ascontiguousarray(w2, dtype=np.float64)
    if w1.ndim != 1 or w2.ndim != 1 or w1.size < 1 or w2.size < 1:
        raise ValueError("w1 / w2 must be 1-D half kernels (centre weight first)")
    F, H, W = movie.shape
    cap = int(max_peaks_per_frame)
    dev = movie.device
    count = torch.zeros(F, dtype=torch.int32, device=dev)
    ncand = torch.zeros(F, dtype=torch.int32, device=dev)
    coords = torch.zeros(F, max(cap, 0), 2, dtype=torch.int32, device=dev)
    values = torch.zeros(F, max(cap, 0), dtype=torch.float32, device=dev)
    dog = torch.empty(F, H, W, dtype=torch.float32, device=dev) if return_dog else None
    wsb = N.lib.mivit_dog_peaks_workspace_bytes(F, H, W, cap, 1 if return_dog else 0)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    N.check(N.lib.mivit_dog_peaks(_p(movie), F, H, W, w1.ctypes.data_as(ctypes.c_void_p), w1.size - 1,
                                  w2.ctypes.data_as(ctypes.c_void_p), w2.size - 1, float(threshold_percentage),
                                  int(min_distance), cap, _p(count), _p(ncand), _p(coords), _p(values), _p(dog), _p(ws),
                                  ws.numel(), _s(movie)), "mivit_dog_peaks")
    worst = int(ncand.max()) if F else 0
    if worst > cap:
        raise RuntimeError(f"dog_peaks: a frame has {worst} peak candidates but max_peaks_per_frame = {cap}; raise "
                           f"max_peaks_per_frame (up to {DOG_PEAKS_MAX_CAPACITY}) or the threshold")
    return count, coords, values, dog


SCORE_PEAKS_MAX_RADIUS = 7


def _camera_args(gain, offset, read_var):
    """The scalars of the photon-counting camera, checked -> (gain, offset, read_var) as floats."""
    import math
    gain, offset, read_var = float(gain), float(offset), float(read_var)
    if not (gain > 0 and math.isfinite(gain)):
        raise ValueError(f"gain must be finite and > 0, got {gain}")
    if not math.isfinite(offset):
        raise ValueError(f"offset must be finite, got {offset}")
    if not (read_var >= 0 and math.isfinite(read_var)):
        raise ValueError(f"read_var must be finite and >= 0, got {read_var}")
    return gain, offset, read_var


def _score_args(name, movie, e, gain, offset, read_var, threshold, cap):
    """The checks the two stages of the likelihood-ratio detector share -> (movie, e as float64, radius, cap)."""
    import math
    import numpy as np
    movie = _frames_f32(movie, name)
    if movie.dim() != 3:
        raise ValueError(f"movie must be [F, H, W], got {tuple(movie.shape)}")
    e = np.ascontiguousarray(e, dtype=np.float64)
    if e.ndim != 1 or e.size % 2 != 1 or not 1 <= e.size // 2 <= SCORE_PEAKS_MAX_RADIUS:
        raise ValueError(f"e must hold the 2 radius + 1 profile values of a radius from 1 to {SCORE_PEAKS_MAX_RADIUS}, got "
                         f"shape {e.shape}")
    r = e.size // 2
    if not (np.all(e > 0) and np.all(e <= 1)):
        raise ValueError("e must lie in (0, 1]")
    if movie.shape[1] <= r or movie.shape[2] <= r:
        raise ValueError(f"frames of {movie.shape[1]} x {movie.shape[2]} are not larger than the radius {r}")
    _camera_args(gain, offset, read_var)
    if not (threshold >= 0 and math.isfinite(threshold)):
        raise ValueError(f"threshold must be finite and >= 0, got {threshold}")
    cap = int(cap)
    if not 1 <= cap <= DOG_PEAKS_MAX_CAPACITY:
        raise ValueError(f"max_peaks_per_frame must be from 1 to {DOG_PEAKS_MAX_CAPACITY}, got {cap}")
    return movie, e, r, cap


def score_peaks(movie: torch.Tensor, e, gain: float = 1.0, offset: float = 0.0, read_var: float = 0.0,
                threshold: float = 0.0, min_distance: int = 3, max_peaks_per_frame: int = 512, return_map: bool = True):
    """Stage 1 of the likelihood-ratio detector (csrc/detect.hip, mivit_score_peaks): the score statistic of "background
    plus a spot centred here" against "background only" at every pixel of movie [F, H, W] (float32 on the GPU, camera units
    as fit_spots_mle), and its local maxima strictly above the absolute threshold.  e: the 2 r + 1 float64 values of the
    pixel-integrated profile, as helpers/tracking.psf_profile builds them -> (count [F] int32, coords [F, cap, 2] int32
    (y, x), values [F, cap] float32, score map [F, H, W] float32 or None), in the layout and order of dog_peaks.  Raises if
    a frame has more candidates than max_peaks_per_frame."""
    gain, offset, read_var, threshold = float(gain), float(offset), float(read_var), float(threshold)
    movie, e, r, cap = _score_args("score_peaks", movie, e, gain, offset, read_var, threshold, max_peaks_per_frame)
    if int(min_distance) != min_distance or not 1 <= min_distance <= 16:
        raise ValueError(f"min_distance must be an integer from 1 to 16, got {min_distance}")
    F, H, W = movie.shape
    dev = movie.device
    count = torch.zeros(F, dtype=torch.int32, device=dev)
    ncand = torch.zeros(F, dtype=torch.int32, device=dev)
    coords = torch.zeros(F, cap, 2, dtype=torch.int32, device=dev)
    values = torch.zeros(F, cap, dtype=torch.float32, device=dev)
    smap = torch.empty(F, H, W, dtype=torch.float32, device=dev) if return_map else None
    wsb = N.lib.mivit_score_peaks_workspace_bytes(F, H, W, cap, 1 if return_map else 0)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    N.check(N.lib.mivit_score_peaks(_p(movie), F, H, W, e.ctypes.data_as(ctypes.c_void_p), r, gain, offset, read_var,
                                    threshold, int(min_distance), cap, _p(count), _p(ncand), _p(coords), _p(values),
                                    _p(smap), _p(ws), ws.numel(), _s(movie)), "mivit_score_peaks")
    worst = int(ncand.max()) if F else 0
    if worst > cap:
        raise RuntimeError(f"score_peaks: a frame has {worst} peak candidates but max_peaks_per_frame = {cap}; raise "
                           f"max_peaks_per_frame (up to {DOG_PEAKS_MAX_CAPACITY}) or lower p_fa")
    return count, coords, values, smap


def lrt_peaks(movie: torch.Tensor, e, gain: float, offset: float, read_var: float, threshold: float, count: torch.Tensor,
              coords: torch.Tensor, values: torch.Tensor):
    """Stage 2 of the likelihood-ratio detector (csrc/detect.hip, mivit_lrt_peaks): the exact Poisson likelihood ratio T of
    mu = theta g + beta against a constant at every candidate that score_peaks returned (count [F] int32, coords [F, cap, 2]
    int32, values [F, cap] float32 on the GPU), kept where T > threshold and compacted per frame in their order, without a
    copy to the host -> (count [F] int32, coords [F, cap, 2] int32, stats [F, cap, 4] float64 (T, photons, background per
    pixel, the stage-1 statistic), status [F, cap] int32: 0 converged, 1 damping exhausted, 2 iteration cap).  Entries past
    count are zero."""
    gain, offset, read_var, threshold = float(gain), float(offset), float(read_var), float(threshold)
    if coords.dim() != 3 or coords.shape[2] != 2:
        raise ValueError(f"coords must be [F, cap, 2], got {tuple(coords.shape)}")
    movie, e, r, cap = _score_args("lrt_peaks", movie, e, gain, offset, read_var, threshold, coords.shape[1])
    F, H, W = movie.shape
    dev = movie.device
    for name, t, dt, shape in (("count", count, torch.int32, (F,)), ("coords", coords, torch.int32, (F, cap, 2)),
                               ("values", values, torch.float32, (F, cap))):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == dt and tuple(t.shape) == shape):
            raise ValueError(f"{name} must be a {dt} tensor of shape {shape} on {dev}")
    count, coords, values = count.contiguous(), coords.contiguous(), values.contiguous()
    kept = torch.zeros(F, dtype=torch.int32, device=dev)
    kcoords = torch.zeros(F, cap, 2, dtype=torch.int32, device=dev)
    stats = torch.zeros(F, cap, 4, dtype=torch.float64, device=dev)
    status = torch.zeros(F, cap, dtype=torch.int32, device=dev)
    N.check(N.lib.mivit_lrt_peaks(_p(movie), F, H, W, e.ctypes.data_as(ctypes.c_void_p), r, gain, offset, read_var, threshold,
                                  cap, _p(count), _p(coords), _p(values), _p(kept), _p(kcoords), _p(stats), _p(status),
                                  _s(movie)), "mivit_lrt_peaks")
    return kept, kcoords, stats, status


def refine_gaussian(patches: torch.Tensor, xtol: float = 1e-11):
    """Five-parameter Gaussian fit of every patch (csrc/tracking.hip, mivit_refine_gaussian): patches [N, P, P] float32 on the
    GPU, P odd, 3 .. 15 -> (params [N, 5] float64 (amplitude, x0, y0, sigma, offset), peak [N] float32 = patch.max(),
    status [N] int32, 0 where the fit converged)."""
    patches = _frames_f32(patches, "refine_gaussian")
    if patches.dim() != 3 or patches.shape[1] != patches.shape[2]:
        raise ValueError(f"patches must be [N, P, P], got {tuple(patches.shape)}")
    n, P, _ = patches.shape
    params = torch.zeros(n, 5, dtype=torch.float64, device=patches.device)
    peak = torch.zeros(n, dtype=torch.float32, device=patches.device)
    status = torch.zeros(n, dtype=torch.int32, device=patches.device)
    N.check(N.lib.mivit_refine_gaussian(_p(patches), n, P, float(xtol), _p(params), _p(peak), _p(status), _s(patches)),
            "mivit_refine_gaussian")
    return params, peak, status


def _spot_fit_args(name, patches, gain, offset, read_var, sigma0, xtol, n_params):
    """What the Poisson fits share: patches [N, P, P], the camera, sigma0 and xtol checked, and the outputs allocated ->
    (patches, (gain, offset, read_var, sigma0, xtol) as floats, (params [N, n_params], crlb [N, n_params], deviance [N],
    status [N], iterations [N]))."""
    patches = _frames_f32(patches, name)
    if patches.dim() != 3 or patches.shape[1] != patches.shape[2]:
        raise ValueError(f"patches must be [N, P, P], got {tuple(patches.shape)}")
    n, P, _ = patches.shape
    gain, offset, read_var = _camera_args(gain, offset, read_var)
    sigma0, xtol = float(sigma0), float(xtol)
    if not 0.2 < sigma0 < P:
        raise ValueError(f"sigma0 must lie in (0.2, {P}), got {sigma0}")
    if not 0 < xtol <= 1.49012e-8:
        raise ValueError(f"xtol must be in (0, 1.49012e-8], got {xtol}")
    dev = patches.device
    out = (torch.zeros(n, n_params, dtype=torch.float64, device=dev), torch.zeros(n, n_params, dtype=torch.float64, device=dev),
           torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
           torch.zeros(n, dtype=torch.int32, device=dev))
    return patches, (gain, offset, read_var, sigma0, xtol), out


def fit_spots_mle(patches: torch.Tensor, gain: float = 1.0, offset: float = 0.0, read_var: float = 0.0, sigma0: float = 1.0,
                  fit_sigma: bool = True, xtol: float = 1e-11):
    """Poisson maximum-likelihood fit of every patch with its Cramer-Rao bound (csrc/localize.hip, mivit_fit_spots_mle):
    patches [N, P, P] float32 on the GPU, P odd, 3 .. 15, in camera units; photons = max((patch - offset) / gain, 0), read_var
    the readout variance in photons^2 -> (params [N, 5] float64 (photons, x0, y0, sigma, background per pixel), crlb [N, 5]
    float64 (variances; NaN where status != 0), deviance [N] float64, status [N] int32 (0 where the fit converged),
    iterations [N] int32).  fit_sigma=False holds sigma at sigma0."""
    patches, scalars, out = _spot_fit_args("fit_spots_mle", patches, gain, offset, read_var, sigma0, xtol, 5)
    n, P, _ = patches.shape
    gain, offset, read_var, sigma0, xtol = scalars
    N.check(N.lib.mivit_fit_spots_mle(_p(patches), n, P, gain, offset, read_var, sigma0, 1 if fit_sigma else 0, xtol,
                                      *map(_p, out), _s(patches)), "mivit_fit_spots_mle")
    return out


def fit_spots_mle2(patches: torch.Tensor, count: torch.Tensor, guess: torch.Tensor, gain: float = 1.0, offset: float = 0.0,
                   read_var: float = 0.0, sigma0: float = 1.0, fit_sigma: bool = True, xtol: float = 1e-11):
    """Joint Poisson maximum-likelihood fit of one or two emitters per patch, one width and one background for both
    (csrc/localize2.hip, mivit_fit_spots_mle2): patches [N, P, P] float32 on the GPU and the camera scalars as fit_spots_mle,
    count [N] int32 (1 or 2 emitters; the caller guarantees it: another value ends with status 3), guess [N, 4] float64 (the
    starting centres x1, y1, x2, y2 in patch coordinates; the last two are not read where count = 1) -> (params [N, 8] float64
    (N1, x1, y1, N2, x2, y2, sigma, background), crlb [N, 8] float64 (variances; NaN where status != 0), deviance [N] float64,
    status [N] int32, iterations [N] int32).  Where count = 1 the entries of emitter 2 are NaN."""
    patches, scalars, out = _spot_fit_args("fit_spots_mle2", patches, gain, offset, read_var, sigma0, xtol, 8)
    n, P, _ = patches.shape
    gain, offset, read_var, sigma0, xtol = scalars
    for t, name, dtype, shape in ((count, "count", torch.int32, (n,)), (guess, "guess", torch.float64, (n, 4))):
        if not torch.is_tensor(t) or t.device != patches.device:
            raise RuntimeError(f"fit_spots_mle2: {name} must be a GPU tensor on the patches' device")
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"fit_spots_mle2: {name} must be {dtype} of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    count, guess = count.contiguous(), guess.contiguous()
    N.check(N.lib.mivit_fit_spots_mle2(_p(patches), _p(count), _p(guess), n, P, gain, offset, read_var, sigma0,
                                       1 if fit_sigma else 0, xtol, *map(_p, out), _s(patches)), "mivit_fit_spots_mle2")
    return out


def spot_neighbours(frame_offsets: torch.Tensor, ys: torch.Tensor, xs: torch.Tensor, reach: int):
    """The nearest other detection of the same frame within a square reach (csrc/localize2.hip, mivit_spot_neighbours): rows
    sorted by frame, frame_offsets [F + 1] int32 over ys, xs [n] int32 (the integer positions), all on the GPU -> (neighbour
    [n] int32: the row with max(|dy|, |dx|) <= reach nearest by squared Euclidean distance, ties to the lower row, -1 if there
    is none; n_neighbours [n] int32: the rows within reach)."""
    for t, name in ((frame_offsets, "frame_offsets"), (ys, "ys"), (xs, "xs")):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError(f"spot_neighbours: {name} must be a GPU tensor")
        if t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError(f"spot_neighbours: {name} must be a 1-D int32 tensor")
    if len(ys) != len(xs) or len(frame_offsets) < 1:
        raise ValueError("spot_neighbours: ys and xs must have one entry per row and frame_offsets at least one entry")
    if int(reach) != reach or reach < 0:
        raise ValueError(f"reach must be an integer >= 0, got {reach}")
    frame_offsets, ys, xs = frame_offsets.contiguous(), ys.contiguous(), xs.contiguous()
    n = len(ys)
    neighbour = torch.full((n,), -1, dtype=torch.int32, device=ys.device)
    within = torch.zeros(n, dtype=torch.int32, device=ys.device)
    N.check(N.lib.mivit_spot_neighbours(_p(frame_offsets), _p(ys), _p(xs), len(frame_offsets) - 1, n, int(reach),
                                        _p(neighbour), _p(within), _s(ys)), "mivit_spot_neighbours")
    return neighbour, within


LINK_MAX_DETECTIONS = 1024


def _link_args(count, cap, movie_start, name):
    if count.dtype != torch.int32 or count.dim() != 1 or count.device.type != "cuda":
        raise ValueError(f"{name}: count must be a 1-D int32 GPU tensor")
    if not 1 <= cap <= LINK_MAX_DETECTIONS:
        raise ValueError(f"{name}: capacity of {cap} detections per frame, the kernel's limit is {LINK_MAX_DETECTIONS} "
                         f"(LINK_MAX_DETECTIONS); detect with max_peaks_per_frame <= {LINK_MAX_DETECTIONS}")
    if movie_start is None:
        return count.contiguous(), None
    ms = torch.as_tensor(movie_start, device=count.device)
    if ms.shape != count.shape:
        raise ValueError(f"{name}: movie_start must have one entry per frame, got {tuple(ms.shape)} for {count.shape[0]} frames")
    return count.contiguous(), (ms != 0).to(torch.uint8).contiguous()


def link_frames(coords: torch.Tensor, count: torch.Tensor, max_distance: float = 15.0, movie_start=None) -> torch.Tensor:
    """Exact linear assignment between the detections of every pair of consecutive frames (csrc/linking.hip,
    mivit_link_frames): coords [F, cap, 2] int32 (y, x) and count [F] int32 on the GPU, as dog_peaks returns them; movie_start
    [F] (optional): a true entry opens a new movie, whose first frame gets no links -> link [F, cap] int32, for every
    detection of frame f the index of its partner in frame f - 1, or -1 (also beyond count[f]).  The full problem is solved,
    then links longer than max_distance are dropped.  cap <= LINK_MAX_DETECTIONS."""
    if coords.dtype != torch.int32 or coords.dim() != 3 or coords.shape[2] != 2 or coords.device.type != "cuda":
        raise ValueError("link_frames: coords must be an int32 GPU tensor [F, cap, 2]")
    F, cap = coords.shape[0], coords.shape[1]
    if count.shape != (F,):
        raise ValueError(f"link_frames: count must be [{F}], got {tuple(count.shape)}")
    count, ms = _link_args(count, cap, movie_start, "link_frames")
    if not float(max_distance) == float(max_distance):
        raise ValueError("link_frames: max_distance is NaN")
    coords = coords.contiguous()
    link = torch.empty(F, cap, dtype=torch.int32, device=coords.device)
    N.check(N.lib.mivit_link_frames(_p(coords), _p(count), _p(ms), F, cap, float(max_distance), _p(link), _s(coords)),
            "mivit_link_frames")
    return link


LINK_MAX_GAP = 8             # csrc/linking.hip: missed frames a gap link may bridge


def _check_max_gap(max_gap, name):
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, float)) or int(max_gap) != max_gap \
            or not 1 <= max_gap <= LINK_MAX_GAP:
        raise ValueError(f"{name}: max_gap must be an integer from 1 to {LINK_MAX_GAP} (LINK_MAX_GAP), got {max_gap!r}")
    return int(max_gap)


def close_gaps(coords: torch.Tensor, count: torch.Tensor, link: torch.Tensor, max_gap: int, max_distance: float = 15.0,
               movie_start=None):
    """Links across missed detections (csrc/linking.hip, mivit_close_gaps): coords [F, cap, 2] int32, count [F] int32 and link
    [F, cap] int32 (link_frames) on the GPU -> (gap_partner [F, cap] int32, gap_frames [F, cap] int32): the start of a track
    at (f, j) continues the track that ended at detection gap_partner[f, j] of frame f - gap_frames[f, j], with
    gap_frames - 1 <= max_gap frames missed in between; -1 / 0 everywhere else.  Passes g = 2 .. max_gap + 1, shortest gaps
    first; per pass and frame the full assignment between the open ends of frame f - g and the open starts of frame f is
    solved as link_frames solves it, then pairs longer than max_distance are dropped and stay open for the later passes.  No
    gap link crosses a movie_start frame.  1 <= max_gap <= LINK_MAX_GAP."""
    if coords.dtype != torch.int32 or coords.dim() != 3 or coords.shape[2] != 2 or coords.device.type != "cuda":
        raise ValueError("close_gaps: coords must be an int32 GPU tensor [F, cap, 2]")
    F, cap = coords.shape[0], coords.shape[1]
    if count.shape != (F,):
        raise ValueError(f"close_gaps: count must be [{F}], got {tuple(count.shape)}")
    if not torch.is_tensor(link) or link.dtype != torch.int32 or link.device.type != "cuda" or link.shape != (F, cap):
        raise ValueError(f"close_gaps: link must be an int32 GPU tensor [{F}, {cap}]")
    count, ms = _link_args(count, cap, movie_start, "close_gaps")
    max_gap = _check_max_gap(max_gap, "close_gaps")
    if not float(max_distance) == float(max_distance):
        raise ValueError("close_gaps: max_distance is NaN")
    coords, link = coords.contiguous(), link.contiguous()
    gap_partner = torch.empty(F, cap, dtype=torch.int32, device=coords.device)
    gap_frames = torch.empty(F, cap, dtype=torch.int32, device=coords.device)
    ws = torch.empty(max(F * cap, 1), dtype=torch.uint8, device=coords.device)
    N.check(N.lib.mivit_close_gaps(_p(coords), _p(count), _p(link), _p(ms), F, cap, max_gap, float(max_distance),
                                   _p(gap_partner), _p(gap_frames), _p(ws), ws.numel(), _s(coords)), "mivit_close_gaps")
    return gap_partner, gap_frames


def chain_tracks(link: torch.Tensor, count: torch.Tensor, movie_start=None, gap_partner=None, gap_frames=None):
    """Track ids from the links (csrc/linking.hip, mivit_chain_tracks): link [F, cap] int32 (link_frames), count [F] int32 ->
    (ids [F, cap] int32, -1 beyond count[f]; lengths [F * cap] int32, the number of positions of track i at index i, 0 beyond
    the last track; n_tracks [1] int32).  Ids are handed out as the reference does: frame 0 (and every movie_start frame) one
    per detection, later a linked detection inherits, an unlinked one takes the next id in ascending detection index.  With
    gap_partner / gap_frames [F, cap] int32 (close_gaps; mivit_chain_tracks_gaps) an unlinked detection with a gap link
    inherits the id of its partner gap_frames frames earlier; lengths keeps counting detections."""
    if link.dtype != torch.int32 or link.dim() != 2 or link.device.type != "cuda":
        raise ValueError("chain_tracks: link must be an int32 GPU tensor [F, cap]")
    F, cap = link.shape
    if count.shape != (F,):
        raise ValueError(f"chain_tracks: count must be [{F}], got {tuple(count.shape)}")
    count, ms = _link_args(count, cap, movie_start, "chain_tracks")
    if (gap_partner is None) != (gap_frames is None):
        raise ValueError("chain_tracks: gap_partner and gap_frames must both be given or both be None")
    for name, t in (("gap_partner", gap_partner), ("gap_frames", gap_frames)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int32 or t.device.type != "cuda"
                              or t.shape != (F, cap)):
            raise ValueError(f"chain_tracks: {name} must be an int32 GPU tensor [{F}, {cap}]")
    link = link.contiguous()
    ids = torch.full((F, cap), -1, dtype=torch.int32, device=link.device)
    lengths = torch.zeros(F * cap, dtype=torch.int32, device=link.device)
    n_tracks = torch.zeros(1, dtype=torch.int32, device=link.device)
    if gap_partner is None:
        N.check(N.lib.mivit_chain_tracks(_p(link), _p(count), _p(ms), F, cap, _p(ids), _p(lengths), _p(n_tracks), _s(link)),
                "mivit_chain_tracks")
    else:
        gap_partner, gap_frames = gap_partner.contiguous(), gap_frames.contiguous()
        N.check(N.lib.mivit_chain_tracks_gaps(_p(link), _p(gap_partner), _p(gap_frames), _p(count), _p(ms), F, cap, LINK_MAX_GAP,
                                              _p(ids), _p(lengths), _p(n_tracks), _s(link)), "mivit_chain_tracks_gaps")
    return ids, lengths, n_tracks


MSD_LDS_ROWS = 4096          # csrc/diffusion.hip: tracks of up to this many rows are staged in LDS


def _dev_tensor(t, dtype, ndim, name, what):
    if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dtype or t.dim() != ndim:
        raise ValueError(f"{name}: {what} must be a {ndim}-D {str(dtype).replace('torch.', '')} GPU tensor")
    return t.contiguous()


def track_msd(pos: torch.Tensor, offsets: torch.Tensor, dt: float = 1.0, max_lag: int = 0, Lmax: int = None):
    """Mean square displacement and both classical estimates of D for every track (csrc/diffusion.hip, mivit_track_msd): pos
    [N, 2] float64 on the GPU, sorted by track and by frame within a track; offsets [n_tracks + 1] int32 (CSR, from 0 to N);
    max_lag 0 means all lags; Lmax the width of the rows (default: the longest track, which costs one copy of a number to the
    host) -> (msd [n_tracks, Lmax] float64, d_lstsq [n_tracks], d_weighted [n_tracks]).  See helpers/msd.track_msd for the
    arithmetic; a track with fewer than two rows gets a zero row and NaN."""
    pos = _dev_tensor(pos, torch.float64, 2, "track_msd", "pos [N, 2]")
    offsets = _dev_tensor(offsets, torch.int32, 1, "track_msd", "offsets [n_tracks + 1]")
    if pos.shape[1] != 2:
        raise ValueError(f"track_msd: pos must be [N, 2], got {tuple(pos.shape)}")
    if offsets.numel() < 1:
        raise ValueError("track_msd: offsets must have n_tracks + 1 entries")
    if int(max_lag) != max_lag or max_lag < 0:
        raise ValueError(f"track_msd: max_lag must be an integer >= 0 (0: all lags), got {max_lag}")
    n, n_tracks = pos.shape[0], offsets.numel() - 1
    if Lmax is None:
        Lmax = int((offsets[1:] - offsets[:-1]).max()) if n_tracks else 0
    if int(Lmax) != Lmax or Lmax < 0:
        raise ValueError(f"track_msd: Lmax must be an integer >= 0, got {Lmax}")
    msd = torch.empty(n_tracks, int(Lmax), dtype=torch.float64, device=pos.device)
    d_lstsq = torch.empty(n_tracks, dtype=torch.float64, device=pos.device)
    d_weighted = torch.empty(n_tracks, dtype=torch.float64, device=pos.device)
    N.check(N.lib.mivit_track_msd(_p(pos), n, _p(offsets), n_tracks, float(dt), int(max_lag), int(Lmax), _p(msd), _p(d_lstsq),
                                  _p(d_weighted), _s(pos)), "mivit_track_msd")
    return msd, d_lstsq, d_weighted


def track_sequences(movie: torch.Tensor, frame: torch.Tensor, y: torch.Tensor, x: torch.Tensor, seq_row: torch.Tensor,
                    seq_len: int, patch_size: int = 7, lo: float = 0.0, denom: float = 1.0, normalize: bool = False):
    """The model's input from the table sorted by track (csrc/diffusion.hip, mivit_track_sequences): movie [F, H, W] float32 on
    the GPU; frame / y / x [N] int32 (rounded positions); seq_row [n_seq] int32, the table row where each window of seq_len
    rows starts -> [n_seq, seq_len, patch_size, patch_size] float32.  Pixels outside the frame read as 0, then (with
    normalize) every pixel becomes (v - lo) / denom in float32; a row whose frame is outside the movie gives a zero patch."""
    movie = _frames_f32(movie, "track_sequences")
    if movie.dim() != 3:
        raise ValueError(f"track_sequences: movie must be [F, H, W], got {tuple(movie.shape)}")
    frame = _dev_tensor(frame, torch.int32, 1, "track_sequences", "frame [N]")
    y = _dev_tensor(y, torch.int32, 1, "track_sequences", "y [N]")
    x = _dev_tensor(x, torch.int32, 1, "track_sequences", "x [N]")
    seq_row = _dev_tensor(seq_row, torch.int32, 1, "track_sequences", "seq_row [n_seq]")
    if not (frame.numel() == y.numel() == x.numel()):
        raise ValueError("track_sequences: frame, y and x must have one entry per row")
    T, P = int(seq_len), int(patch_size)
    if T != seq_len or T < 1:
        raise ValueError(f"track_sequences: seq_len must be an integer >= 1, got {seq_len}")
    if P != patch_size or P % 2 != 1 or not 3 <= P <= 15:
        raise ValueError(f"track_sequences: patch_size must be odd and from 3 to 15, got {patch_size}")
    if normalize and not (float(denom) != 0.0 and float(denom) == float(denom) and float(lo) == float(lo)):
        raise ValueError(f"track_sequences: cannot normalise with lo = {lo}, denom = {denom}")
    F, H, W = movie.shape
    n_seq = seq_row.numel()
    seq = torch.empty(n_seq, T, P, P, dtype=torch.float32, device=movie.device)
    N.check(N.lib.mivit_track_sequences(_p(movie), F, H, W, _p(frame), _p(y), _p(x), frame.numel(), _p(seq_row), n_seq, T, P,
                                        float(lo), float(denom), 1 if normalize else 0, _p(seq), _s(movie)),
            "mivit_track_sequences")
    return seq


FGN_MAX_T = 2048             # csrc/fbm.hip: steps of a trajectory whose recursion state fits in LDS
FGN_MAX_C = 4


def fgn(z: torch.Tensor, gamma: torch.Tensor, gamma_row: torch.Tensor) -> torch.Tensor:
    """Fractional Gaussian noise (csrc/fbm.hip, mivit_fgn): z [N, T, C] float64 standard normals, 1 <= C <= FGN_MAX_C, gamma
    [U, T] float64 autocovariance rows (helpers/generation.fgn_autocovariance), gamma_row [N] int32 in [0, U), all on the GPU
    -> [N, T, C] float64, the Cholesky factor of gamma's Toeplitz matrix applied to every trajectory and axis.  T <=
    FGN_MAX_T.  See include/mivit_hip.h for the recursion and helpers/generation.fractional_gaussian_noise for the front end."""
    z = _dev_tensor(z, torch.float64, 3, "fgn", "z [N, T, C]")
    gamma = _dev_tensor(gamma, torch.float64, 2, "fgn", "gamma [U, T]")
    gamma_row = _dev_tensor(gamma_row, torch.int32, 1, "fgn", "gamma_row [N]")
    n, T, C = z.shape
    U = gamma.shape[0]
    if not 1 <= C <= FGN_MAX_C:
        raise ValueError(f"fgn: z holds {C} axes, 1 .. {FGN_MAX_C} (FGN_MAX_C) are supported")
    if T > FGN_MAX_T:
        raise ValueError(f"fgn: T = {T} steps, the kernel's limit is {FGN_MAX_T} (FGN_MAX_T)")
    if gamma.shape[1] != T or gamma_row.numel() != n:
        raise ValueError(f"fgn: gamma must be [U, {T}] and gamma_row [{n}], got {tuple(gamma.shape)} and {tuple(gamma_row.shape)}")
    if n and T and (U < 1 or int(gamma_row.min()) < 0 or int(gamma_row.max()) >= U):
        raise ValueError(f"fgn: gamma_row must lie in [0, {U})")
    out = torch.empty_like(z)
    N.check(N.lib.mivit_fgn(_p(z), _p(gamma), _p(gamma_row), n, T, C, U, _p(out), _s(z)), "mivit_fgn")
    return out


GEOM_CHUNK_T = 2048          # csrc/confine.hip: steps per pass through LDS (no limit on T)
GEOM_MAX_EDGES = 512         # edges of one polyline, staged in LDS
GEOM_MODES = {"clamp": 0, "reflect": 1}


def map_displacements(disp: torch.Tensor, s0: torch.Tensor, geom_of: torch.Tensor, verts: torch.Tensor, lengths: torch.Tensor,
                      vert_offsets: torch.Tensor, totals: torch.Tensor, mode):
    """Displacements along polylines -> positions (csrc/confine.hip, mivit_map_displacements): disp [N, T] float64, s0 [N]
    float64 start arcs, geom_of [N] int32 in [0, G); the packed geometries of helpers/geometry.pack_geometries: verts [V, 2]
    float64, lengths [V] float64, vert_offsets [G + 1] int32, totals [G] float64, all on the GPU; mode "clamp" / 0 (the
    reference: the arc is clamped to [0, total] after every step) or "reflect" / 1 (folded back at both ends) -> (pos [N, T, 2]
    float64, arc [N, T] float64, edge [N, T] int32).  No limit on T; a geometry has at most GEOM_MAX_EDGES edges.  See
    include/mivit_hip.h for the arithmetic and helpers/geometry.map_displacements for the front end."""
    disp = _dev_tensor(disp, torch.float64, 2, "map_displacements", "disp [N, T]")
    s0 = _dev_tensor(s0, torch.float64, 1, "map_displacements", "s0 [N]")
    geom_of = _dev_tensor(geom_of, torch.int32, 1, "map_displacements", "geom_of [N]")
    verts = _dev_tensor(verts, torch.float64, 2, "map_displacements", "verts [V, 2]")
    lengths = _dev_tensor(lengths, torch.float64, 1, "map_displacements", "lengths [V]")
    vert_offsets = _dev_tensor(vert_offsets, torch.int32, 1, "map_displacements", "vert_offsets [G + 1]")
    totals = _dev_tensor(totals, torch.float64, 1, "map_displacements", "totals [G]")
    if mode not in GEOM_MODES and not (isinstance(mode, int) and not isinstance(mode, bool) and mode in GEOM_MODES.values()):
        raise ValueError(f"map_displacements: mode must be one of {sorted(GEOM_MODES)} (or 0 / 1), got {mode!r}")
    mode = GEOM_MODES.get(mode, mode)
    n, T = disp.shape
    V, G = verts.shape[0], totals.numel()
    if s0.numel() != n or geom_of.numel() != n:
        raise ValueError(f"map_displacements: s0 and geom_of must be [{n}], got {tuple(s0.shape)} and {tuple(geom_of.shape)}")
    if verts.shape[1] != 2 or lengths.numel() != V or vert_offsets.numel() != G + 1:
        raise ValueError(f"map_displacements: need verts [V, 2], lengths [V], vert_offsets [G + 1] and totals [G], got "
                         f"{tuple(verts.shape)}, {tuple(lengths.shape)}, {tuple(vert_offsets.shape)} and {tuple(totals.shape)}")
    if n and T:
        if G < 1:
            raise ValueError(f"map_displacements: no geometry for {n} particles")
        vo = vert_offsets.cpu()
        nv = vo[1:] - vo[:-1]
        if int(vo[0]) != 0 or int(vo[-1]) != V or int(nv.min()) < 2:
            raise ValueError(f"map_displacements: vert_offsets must rise from 0 to V = {V} with at least two vertices per geometry")
        if int(nv.max()) - 1 > GEOM_MAX_EDGES:
            raise ValueError(f"map_displacements: a geometry has {int(nv.max()) - 1} edges, the kernel's limit is "
                             f"{GEOM_MAX_EDGES} (GEOM_MAX_EDGES)")
        if int(geom_of.min()) < 0 or int(geom_of.max()) >= G:
            raise ValueError(f"map_displacements: geom_of must lie in [0, {G})")
    return _map_displacements_checked(disp, s0, geom_of, verts, lengths, vert_offsets, totals, mode)


def _map_displacements_checked(disp, s0, geom_of, verts, lengths, vert_offsets, totals, mode: int, out=None):
    """map_displacements for contiguous GPU tensors of the right kinds and shapes whose vert_offsets and geom_of the caller has
    already checked (helpers/geometry.map_displacements checks them on the host copies it packs from): allocation and launch,
    nothing is read back.  out: (pos, arc, edge) to write into instead of allocating.  The kernel clamps every index it reads,
    so an unchecked value can give a wrong position but cannot address out of bounds."""
    n, T = disp.shape
    pos, arc, edge = out if out is not None else (torch.empty(n, T, 2, dtype=torch.float64, device=disp.device),
                                                  torch.empty(n, T, dtype=torch.float64, device=disp.device),
                                                  torch.empty(n, T, dtype=torch.int32, device=disp.device))
    N.check(N.lib.mivit_map_displacements(_p(disp), _p(s0), _p(geom_of), _p(verts), _p(lengths), _p(vert_offsets), _p(totals), n, T,
                                          totals.numel(), verts.shape[0], mode, _p(pos), _p(arc), _p(edge), _s(disp)),
            "mivit_map_displacements")
    return pos, arc, edge


# csrc/segment.hip: rows of a track whose recurrence state fits in LDS (the variance model 20 B a row, 81 920 B at the limit;
# the transport model 36 B a row, 147 456 B)
SEG_MAX_LEN = 4096
TRANSPORT_MAX_LEN = SEG_MAX_LEN
MARKOV_MAX_K = 8             # csrc/segment.hip: states of mivit_markov_states; csrc/hmm.hip: of mivit_hmm_estep / _viterbi


def _seg_tensor(t, dtype, ndim, name, what):
    """_dev_tensor that takes no copy: a non-contiguous tensor is an error (the helpers pass contiguous ones)."""
    if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dtype or t.dim() != ndim or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous {ndim}-D {str(dtype).replace('torch.', '')} GPU tensor")
    return t


def _partition_args(name, limit_name, pos, offsets, min_len, penalty, min_var):
    """What segment_tracks and segment_transport check alike -> (N, n_tracks, the rows of the longest track: read back from
    offsets, 0 without a track)."""
    _seg_tensor(pos, torch.float64, 2, name, "pos [N, 2]")
    _seg_tensor(offsets, torch.int32, 1, name, "offsets [n_tracks + 1]")
    if pos.shape[1] != 2:
        raise ValueError(f"{name}: pos must be [N, 2], got {tuple(pos.shape)}")
    if offsets.numel() < 1:
        raise ValueError(f"{name}: offsets must have n_tracks + 1 entries")
    if isinstance(min_len, bool) or int(min_len) != min_len or min_len < 2:
        raise ValueError(f"{name}: min_len must be an integer >= 2, got {min_len}")
    if not float(penalty) >= 0.0:
        raise ValueError(f"{name}: penalty must be >= 0, got {penalty}")
    if not 0.0 < float(min_var) < float("inf"):
        raise ValueError(f"{name}: min_var must be positive and finite, got {min_var}")
    n, n_tracks = pos.shape[0], offsets.numel() - 1
    if n_tracks == 0:
        return n, 0, 0
    off = offsets.cpu()
    if int(off[0]) != 0 or int(off[-1]) != n or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"{name}: offsets must rise from 0 to the number of rows {n}")
    max_len = int((off[1:] - off[:-1]).max())
    if max_len > SEG_MAX_LEN:
        raise ValueError(f"{name}: a track of {max_len} rows, the kernel's limit is {SEG_MAX_LEN} ({limit_name})")
    return n, n_tracks, max_len


def _stretch_stats_args(name, pos, seg_offsets, seg_track_end, dt, blur):
    """What segment_stats and transport_stats check alike -> n_seg."""
    _seg_tensor(pos, torch.float64, 2, name, "pos [N, 2]")
    _seg_tensor(seg_offsets, torch.int32, 1, name, "seg_offsets [n_seg + 1]")
    _seg_tensor(seg_track_end, torch.int32, 1, name, "seg_track_end [n_seg]")
    if pos.shape[1] != 2:
        raise ValueError(f"{name}: pos must be [N, 2], got {tuple(pos.shape)}")
    if seg_offsets.numel() != seg_track_end.numel() + 1:
        raise ValueError(f"{name}: seg_offsets must have one entry more than seg_track_end, got {seg_offsets.numel()} and "
                         f"{seg_track_end.numel()}")
    if not 0.0 < float(dt) < float("inf"):
        raise ValueError(f"{name}: dt must be positive and finite, got {dt}")
    if not 0.0 <= float(blur) <= 0.25:
        raise ValueError(f"{name}: the blur coefficient must lie in [0, 1/4], got {blur}")
    return seg_track_end.numel()


def segment_tracks(pos: torch.Tensor, offsets: torch.Tensor, min_len: int = 4, penalty: float = 3.0, min_var: float = 1e-12):
    """The optimal partition of every track into stretches of constant step variance (csrc/segment.hip,
    mivit_segment_tracks): pos [N, 2] float64 on the GPU, sorted by track and by frame; offsets [n_tracks + 1] int32 (CSR, from
    0 to N) -> (seg_start [N] int32, 1 on the first row of every segment; cost [n_tracks] float64, NaN for a track without an
    increment).  A track has at most SEG_MAX_LEN rows.  The longest track is read back (one number) to size the kernel's LDS.
    See include/mivit_hip.h for the recurrence and helpers/msd.segment_tracks for the front end."""
    n, n_tracks, max_len = _partition_args("segment_tracks", "SEG_MAX_LEN", pos, offsets, min_len, penalty, min_var)
    seg_start = torch.zeros(n, dtype=torch.int32, device=pos.device)
    cost = torch.empty(n_tracks, dtype=torch.float64, device=pos.device)
    if n_tracks == 0:
        return seg_start, cost
    N.check(N.lib.mivit_segment_tracks(_p(pos), n, _p(offsets), n_tracks, max_len, int(min_len), float(penalty), float(min_var),
                                       _p(seg_start), _p(cost), _s(pos)), "mivit_segment_tracks")
    return seg_start, cost


def segment_stats(pos: torch.Tensor, seg_offsets: torch.Tensor, seg_track_end: torch.Tensor, dt: float = 1.0, blur: float = 0.0):
    """One row of estimates per segment (csrc/segment.hip, mivit_segment_stats): pos [N, 2] float64 on the GPU, seg_offsets
    [n_seg + 1] int32 (the CSR of the segments over the rows), seg_track_end [n_seg] int32 (the row at which each segment's
    track ends), blur the motion-blur coefficient R in [0, 1/4] -> (D_cve, D_mle, sigma2 [n_seg] float64, n_increments [n_seg]
    int32).  See include/mivit_hip.h for the arithmetic."""
    n_seg = _stretch_stats_args("segment_stats", pos, seg_offsets, seg_track_end, dt, blur)
    d_cve, d_mle, sigma2 = (torch.empty(n_seg, dtype=torch.float64, device=pos.device) for _ in range(3))
    n_inc = torch.empty(n_seg, dtype=torch.int32, device=pos.device)
    N.check(N.lib.mivit_segment_stats(_p(pos), pos.shape[0], _p(seg_offsets), _p(seg_track_end), n_seg, float(dt), float(blur),
                                      _p(d_cve), _p(d_mle), _p(sigma2), _p(n_inc), _s(pos)), "mivit_segment_stats")
    return d_cve, d_mle, sigma2, n_inc


def markov_states(u: torch.Tensor, p0: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """The state paths of a Markov chain from uniform numbers (csrc/segment.hip, mivit_markov_states): u [N, T], p0 [K] and M
    [K, K] float64 on the GPU, 1 <= K <= MARKOV_MAX_K -> state [N, T] int32.  See include/mivit_hip.h and
    helpers/generation.markov_states for the front end, which checks that p0 and the rows of M are distributions."""
    u = _seg_tensor(u, torch.float64, 2, "markov_states", "u [N, T]")
    p0 = _seg_tensor(p0, torch.float64, 1, "markov_states", "p0 [K]")
    M = _seg_tensor(M, torch.float64, 2, "markov_states", "M [K, K]")
    K = p0.numel()
    if not 1 <= K <= MARKOV_MAX_K:
        raise ValueError(f"markov_states: {K} states, 1 .. {MARKOV_MAX_K} (MARKOV_MAX_K) are supported")
    if tuple(M.shape) != (K, K):
        raise ValueError(f"markov_states: M must be [{K}, {K}], got {tuple(M.shape)}")
    n, T = u.shape
    state = torch.empty(n, T, dtype=torch.int32, device=u.device)
    N.check(N.lib.mivit_markov_states(_p(u), _p(p0), _p(M), n, T, K, _p(state), _s(u)), "mivit_markov_states")
    return state


def _hmm_args(name, pos, offsets, v, A, pi):
    """The checks both hidden-Markov wrappers share -> (n, n_tracks, K); every rejection is a ValueError before any launch."""
    pos = _seg_tensor(pos, torch.float64, 2, name, "pos [N, 2]")
    offsets = _seg_tensor(offsets, torch.int32, 1, name, "offsets [n_tracks + 1]")
    v = _seg_tensor(v, torch.float64, 1, name, "v [K]")
    A = _seg_tensor(A, torch.float64, 2, name, "A [K, K]")
    pi = _seg_tensor(pi, torch.float64, 1, name, "pi [K]")
    if pos.shape[1] != 2:
        raise ValueError(f"{name}: pos must be [N, 2], got {tuple(pos.shape)}")
    if offsets.numel() < 1:
        raise ValueError(f"{name}: offsets must have n_tracks + 1 entries")
    K = v.numel()
    if not 1 <= K <= MARKOV_MAX_K:
        raise ValueError(f"{name}: {K} states, 1 .. {MARKOV_MAX_K} (MARKOV_MAX_K) are supported")
    if tuple(A.shape) != (K, K):
        raise ValueError(f"{name}: A must be [{K}, {K}], got {tuple(A.shape)}")
    if pi.numel() != K:
        raise ValueError(f"{name}: pi must be [{K}], got {tuple(pi.shape)}")
    if len({t.device for t in (pos, offsets, v, A, pi)}) != 1:
        raise ValueError(f"{name}: all tensors must be on one device")
    n, n_tracks = pos.shape[0], offsets.numel() - 1
    if n_tracks:
        off = offsets.cpu()
        if int(off[0]) != 0 or int(off[-1]) != n or bool((off[1:] < off[:-1]).any()):
            raise ValueError(f"{name}: offsets must rise from 0 to the number of rows {n}")
    elif n:
        raise ValueError(f"{name}: offsets must rise from 0 to the number of rows {n}")
    return n, n_tracks, K


def hmm_estep(pos: torch.Tensor, offsets: torch.Tensor, v: torch.Tensor, A: torch.Tensor, pi: torch.Tensor):
    """One E-step of the hidden Markov model over the increments of all tracks (csrc/hmm.hip, mivit_hmm_estep): pos [N, 2]
    float64 on the GPU, sorted by track and by frame; offsets [n_tracks + 1] int32 (CSR, from 0 to N); v [K] the per-axis
    increment variance of every state, A [K, K] the transition probabilities, pi [K] the initial distribution, float64, 1 <=
    K <= MARKOV_MAX_K -> (gamma [N, K], state [N] int32, xi [n_tracks, K, K], g_sum, gq_sum, g_first [n_tracks, K], loglik
    [n_tracks]).  A track has no maximum length.  See include/mivit_hip.h for the arithmetic and helpers/msd.
    fit_diffusion_states for the front end."""
    n, n_tracks, K = _hmm_args("hmm_estep", pos, offsets, v, A, pi)
    f64 = dict(dtype=torch.float64, device=pos.device)
    gamma, ws = torch.empty(n, K, **f64), torch.empty(n, K, **f64)
    state = torch.empty(n, dtype=torch.int32, device=pos.device)
    xi = torch.empty(n_tracks, K, K, **f64)
    g_sum, gq_sum, g_first = (torch.empty(n_tracks, K, **f64) for _ in range(3))
    loglik = torch.empty(n_tracks, **f64)
    N.check(N.lib.mivit_hmm_estep(_p(pos), n, _p(offsets), n_tracks, K, _p(v), _p(A), _p(pi), _p(gamma), _p(state), _p(xi),
                                  _p(g_sum), _p(gq_sum), _p(g_first), _p(loglik), _p(ws), _s(pos)), "mivit_hmm_estep")
    return gamma, state, xi, g_sum, gq_sum, g_first, loglik


def hmm_viterbi(pos: torch.Tensor, offsets: torch.Tensor, v: torch.Tensor, A: torch.Tensor, pi: torch.Tensor):
    """The most probable state path of every track under the same model (csrc/hmm.hip, mivit_hmm_viterbi); arguments as
    hmm_estep -> (state [N] int32, -1 on a one-row track; logp [n_tracks] float64, the path's log-probability up to the
    constant -T log(2 pi), NaN for a track without an increment).  The logarithms of v, A and pi are taken here, in torch: the
    kernel adds and compares only.  See include/mivit_hip.h."""
    n, n_tracks, K = _hmm_args("hmm_viterbi", pos, offsets, v, A, pi)
    state = torch.empty(n, dtype=torch.int32, device=pos.device)
    logp = torch.empty(n_tracks, dtype=torch.float64, device=pos.device)
    bp = torch.empty(n, 8, dtype=torch.uint8, device=pos.device)
    logv, logA, logpi = torch.log(v), torch.log(A), torch.log(pi)
    N.check(N.lib.mivit_hmm_viterbi(_p(pos), n, _p(offsets), n_tracks, K, _p(v), _p(logv), _p(logA), _p(logpi), _p(state),
                                    _p(logp), _p(bp), _s(pos)), "mivit_hmm_viterbi")
    return state, logp


def _track_ml_args(name, pos, offsets, var, frames, use, dt, check=None):
    """The checks that the per-track maximum-likelihood fits share (track_diffusion_ml, track_fbm_*, track_confined_*): shapes,
    dtypes, one device, dt, then `check()`, the caller's own checks of its scalars, and last the offsets, which are read back
    -> (pos, offsets, var, frames, use, N, n)"""
    pos = _seg_tensor(pos, torch.float64, 2, name, "pos [N, 2]")
    offsets = _seg_tensor(offsets, torch.int32, 1, name, "offsets [n + 1]")
    if pos.shape[1] != 2:
        raise ValueError(f"{name}: pos must be [N, 2], got {tuple(pos.shape)}")
    if offsets.numel() < 1:
        raise ValueError(f"{name}: offsets must have n + 1 entries")
    n_rows, n = pos.shape[0], offsets.numel() - 1
    given = [pos, offsets]
    if var is not None:
        var = _seg_tensor(var, torch.float64, 2, name, "var [N, 2]")
        if tuple(var.shape) != (n_rows, 2):
            raise ValueError(f"{name}: var must be [{n_rows}, 2], got {tuple(var.shape)}")
        given.append(var)
    if frames is not None:
        frames = _seg_tensor(frames, torch.int32, 1, name, "frames [N]")
        if frames.numel() != n_rows:
            raise ValueError(f"{name}: frames must be [{n_rows}], got {tuple(frames.shape)}")
        given.append(frames)
    if use is not None:
        if torch.is_tensor(use) and use.dtype == torch.bool:
            use = use.view(torch.uint8)
        use = _seg_tensor(use, torch.uint8, 1, name, "use [N] (bool or uint8)")
        if use.numel() != n_rows:
            raise ValueError(f"{name}: use must be [{n_rows}], got {tuple(use.shape)}")
        given.append(use)
    if len({t.device for t in given}) != 1:
        raise ValueError(f"{name}: all tensors must be on one device")
    if not 0.0 < float(dt) < float("inf"):
        raise ValueError(f"{name}: dt must be positive and finite, got {dt}")
    if check is not None:
        check(n)
    if n:
        off = offsets.cpu()
        if int(off[0]) != 0 or int(off[-1]) != n_rows or bool((off[1:] < off[:-1]).any()):
            raise ValueError(f"{name}: offsets must rise from 0 to the number of rows {n_rows}")
    elif n_rows:
        raise ValueError(f"{name}: offsets must rise from 0 to the number of rows {n_rows}")
    return pos, offsets, var, frames, use, n_rows, n


def track_diffusion_ml(pos: torch.Tensor, offsets: torch.Tensor, var=None, frames=None, use=None, dt: float = 1.0,
                       blur: float = 0.0):
    """The maximum-likelihood diffusion coefficient of every row range with its standard error (csrc/likelihood.hip,
    mivit_track_diffusion_ml): pos [N, 2] float64 on the GPU (y, x); offsets [n + 1] int32 (CSR, from 0 to N: tracks, segments
    or runs); var [N, 2] float64, the variance of every coordinate (None: zeros); frames [N] int32, rising within a range
    (None: consecutive); use [N] bool or uint8 (None: every row); blur the motion-blur coefficient R in [0, 1/4] -> (D, D_std,
    loglik [n] float64, n_increments, status [n] int32).  A range has no maximum length.  offsets are read back to be
    checked: every rejection is a ValueError before any launch.  See include/mivit_hip.h for the arithmetic and the status
    codes and helpers/msd.estimate_diffusion_ml for the front end."""
    name = "track_diffusion_ml"

    def check(n):
        if not 0.0 <= float(blur) <= 0.25:
            raise ValueError(f"{name}: the blur coefficient must lie in [0, 1/4], got {blur}")

    pos, offsets, var, frames, use, n_rows, n = _track_ml_args(name, pos, offsets, var, frames, use, dt, check)
    D, D_std, loglik = (torch.empty(n, dtype=torch.float64, device=pos.device) for _ in range(3))
    n_inc, status = (torch.empty(n, dtype=torch.int32, device=pos.device) for _ in range(2))
    N.check(N.lib.mivit_track_diffusion_ml(_p(pos), _p(var), _p(frames), _p(use), n_rows, _p(offsets), n, float(dt),
                                           float(blur), _p(D), _p(D_std), _p(loglik), _p(n_inc), _p(status), _s(pos)),
            "mivit_track_diffusion_ml")
    return D, D_std, loglik, n_inc, status


FBM_ML_MAX_ROWS = 129        # csrc/fbm_ml.hip: usable rows of a range (128 increments: the packed triangle fills the LDS)
FBM_ML_MAX_SPAN = 1199       # csrc/fbm_ml.hip: largest - smallest usable frame of a range (the table of the structure function)
FBM_ML_WS_BYTES = 640        # csrc/fbm_ml.hip: workspace of mivit_track_fbm_ml per range


def _fbm_ml_check(name, exposure):
    """the checks of their own that track_fbm_loglik and track_fbm_ml hand to _track_ml_args"""
    def check(n):
        if not 0.0 <= float(exposure) <= 1.0:
            raise ValueError(f"{name}: the exposure must lie in [0, 1], got {exposure}")
        if n > 1 << 24:
            raise ValueError(f"{name}: {n} ranges, at most {1 << 24} in one call")
    return check


def track_fbm_loglik(pos: torch.Tensor, offsets: torch.Tensor, alpha: torch.Tensor, D: torch.Tensor, var=None, frames=None,
                     use=None, dt: float = 1.0, exposure: float = 0.0):
    """The exact log-likelihood of every row range under fractional Brownian motion seen through an exposure and
    localisation noise of known variance (csrc/fbm_ml.hip, mivit_track_fbm_loglik): pos, offsets, var, frames, use, dt as
    track_diffusion_ml; alpha [n], D [n] float64 the parameters of every range; exposure in [0, 1] -> (loglik [n] float64,
    n_increments, status [n] int32).  A range may have at most FBM_ML_MAX_ROWS usable rows over at most FBM_ML_MAX_SPAN frames
    (status 5).  See include/mivit_hip.h for the arithmetic and the status codes and helpers/msd.fbm_loglik for the front end."""
    name = "track_fbm_loglik"
    pos, offsets, var, frames, use, n_rows, n = _track_ml_args(name, pos, offsets, var, frames, use, dt,
                                                               _fbm_ml_check(name, exposure))
    alpha = _seg_tensor(alpha, torch.float64, 1, name, "alpha [n]")
    D = _seg_tensor(D, torch.float64, 1, name, "D [n]")
    if alpha.numel() != n or D.numel() != n or alpha.device != pos.device or D.device != pos.device:
        raise ValueError(f"{name}: alpha and D must be [{n}] on the device of pos, got {tuple(alpha.shape)} and {tuple(D.shape)}")
    loglik = torch.empty(n, dtype=torch.float64, device=pos.device)
    n_inc, status = (torch.empty(n, dtype=torch.int32, device=pos.device) for _ in range(2))
    N.check(N.lib.mivit_track_fbm_loglik(_p(pos), _p(var), _p(frames), _p(use), n_rows, _p(offsets), n, float(dt), float(exposure),
                                         _p(alpha), _p(D), _p(loglik), _p(n_inc), _p(status), _s(pos)), "mivit_track_fbm_loglik")
    return loglik, n_inc, status


def track_fbm_ml(pos: torch.Tensor, offsets: torch.Tensor, var=None, frames=None, use=None, dt: float = 1.0, exposure: float = 0.0):
    """The maximum-likelihood anomalous exponent and generalised diffusion coefficient of every row range with their standard
    errors (csrc/fbm_ml.hip, mivit_track_fbm_ml): the arguments of track_diffusion_ml with exposure in [0, 1] in the place of
    blur -> (alpha, alpha_std, D, D_std, corr, loglik [n] float64, n_increments, status [n] int32).  The whole search (20
    rounds of 64 candidates a range) is queued on the stream without a host synchronisation; the workspace (FBM_ML_WS_BYTES a
    range) is allocated here.  A range may have at most FBM_ML_MAX_ROWS usable rows over at most FBM_ML_MAX_SPAN frames (status
    5).  See include/mivit_hip.h for the arithmetic and the status codes and helpers/msd.estimate_anomalous_ml for the front end."""
    name = "track_fbm_ml"
    pos, offsets, var, frames, use, n_rows, n = _track_ml_args(name, pos, offsets, var, frames, use, dt,
                                                               _fbm_ml_check(name, exposure))
    outs = [torch.empty(n, dtype=torch.float64, device=pos.device) for _ in range(6)]
    n_inc, status = (torch.empty(n, dtype=torch.int32, device=pos.device) for _ in range(2))
    ws = torch.empty(max(n, 1) * FBM_ML_WS_BYTES // 8, dtype=torch.float64, device=pos.device)
    N.check(N.lib.mivit_track_fbm_ml(_p(pos), _p(var), _p(frames), _p(use), n_rows, _p(offsets), n, float(dt), float(exposure),
                                     *(_p(o) for o in outs), _p(n_inc), _p(status), _p(ws), ws.numel() * 8, _s(pos)),
            "mivit_track_fbm_ml")
    return (*outs, n_inc, status)


def track_confined_ml(pos: torch.Tensor, offsets: torch.Tensor, var=None, frames=None, use=None, dt: float = 1.0):
    """The maximum-likelihood confinement radius of every row range with error bars (csrc/confined_ml.hip,
    mivit_track_confined_ml): diffusion in a harmonic well (an isotropic Ornstein-Uhlenbeck process) seen at instantaneous
    exposure (motion blur is not modelled) through noise of known variance; the arguments of track_diffusion_ml without blur
    -> (D_conf, D_conf_std, radius, radius_std, lambda, lambda_std, corr [n] float64, centre, centre_std [n, 2] float64 (y, x),
    loglik [n] float64, n_increments, status [n] int32).  One launch, one wave per range, no workspace; a range has no maximum
    length.  See include/mivit_hip.h for the arithmetic and the status codes and helpers/msd.estimate_confinement_ml for the
    front end."""
    name = "track_confined_ml"
    pos, offsets, var, frames, use, n_rows, n = _track_ml_args(name, pos, offsets, var, frames, use, dt)
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=pos.device)         # noqa: E731
    outs = [f64(n) for _ in range(7)] + [f64(n, 2), f64(n, 2), f64(n)]
    n_inc, status = (torch.empty(n, dtype=torch.int32, device=pos.device) for _ in range(2))
    N.check(N.lib.mivit_track_confined_ml(_p(pos), _p(var), _p(frames), _p(use), n_rows, _p(offsets), n, float(dt),
                                          *(_p(o) for o in outs), _p(n_inc), _p(status), _s(pos)), "mivit_track_confined_ml")
    return (*outs, n_inc, status)


def track_confined_loglik(pos: torch.Tensor, offsets: torch.Tensor, D: torch.Tensor, s2: torch.Tensor, centre=None, var=None,
                          frames=None, use=None, dt: float = 1.0) -> torch.Tensor:
    """The exact log-likelihood of every row range under confined diffusion at given parameters (csrc/confined_ml.hip,
    mivit_track_confined_loglik): pos, offsets, var, frames, use, dt as track_diffusion_ml; D [n], s2 [n] float64 the diffusion
    coefficient and the stationary variance per axis of every range; centre [n, 2] float64 (y, x), or None for the centre
    that maximises the likelihood -> loglik [n] float64 (NaN without an increment or where D or s2 is not positive and finite,
    -inf for a rejected candidate).  The exposure is instantaneous.  See include/mivit_hip.h for the arithmetic and
    helpers/msd.confined_loglik for the front end."""
    name = "track_confined_loglik"
    pos, offsets, var, frames, use, n_rows, n = _track_ml_args(name, pos, offsets, var, frames, use, dt)
    D = _seg_tensor(D, torch.float64, 1, name, "D [n]")
    s2 = _seg_tensor(s2, torch.float64, 1, name, "s2 [n]")
    if D.numel() != n or s2.numel() != n or D.device != pos.device or s2.device != pos.device:
        raise ValueError(f"{name}: D and s2 must be [{n}] on the device of pos, got {tuple(D.shape)} and {tuple(s2.shape)}")
    if centre is not None:
        centre = _seg_tensor(centre, torch.float64, 2, name, "centre [n, 2]")
        if tuple(centre.shape) != (n, 2) or centre.device != pos.device:
            raise ValueError(f"{name}: centre must be [{n}, 2] on the device of pos, got {tuple(centre.shape)}")
    loglik = torch.empty(n, dtype=torch.float64, device=pos.device)
    N.check(N.lib.mivit_track_confined_loglik(_p(pos), _p(var), _p(frames), _p(use), n_rows, _p(offsets), n, float(dt), _p(D),
                                              _p(s2), _p(centre), _p(loglik), _s(pos)), "mivit_track_confined_loglik")
    return loglik


def _directed_ml_check(name, blur):
    """the check of their own that track_directed_ml and track_directed_loglik hand to _track_ml_args"""
    def check(n):
        if not 0.0 <= float(blur) <= 0.25:
            raise ValueError(f"{name}: the blur coefficient must lie in [0, 1/4], got {blur}")
    return check


def track_directed_ml(pos: torch.Tensor, offsets: torch.Tensor, var=None, frames=None, use=None, dt: float = 1.0,
                      blur: float = 0.0):
    """The maximum-likelihood velocity and diffusion coefficient of every row range under directed motion, with error bars
    (csrc/directed_ml.hip, mivit_track_directed_ml): the model of track_diffusion_ml about a mean velocity * gap * dt, the
    velocity of each axis profiled out in closed form; the arguments of track_diffusion_ml -> (D, D_std [n] float64, velocity,
    velocity_std [n, 2] float64 (y, x) in pixels per unit of dt, loglik [n] float64, n_increments, status [n] int32).  One
    launch, one wave per range, no workspace; a range has no maximum length.  See include/mivit_hip.h for the arithmetic and
    the status codes and helpers/msd.estimate_directed_ml for the front end."""
    name = "track_directed_ml"
    pos, offsets, var, frames, use, n_rows, n = _track_ml_args(name, pos, offsets, var, frames, use, dt,
                                                               _directed_ml_check(name, blur))
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=pos.device)         # noqa: E731
    D, D_std, v, v_std, loglik = f64(n), f64(n), f64(n, 2), f64(n, 2), f64(n)
    n_inc, status = (torch.empty(n, dtype=torch.int32, device=pos.device) for _ in range(2))
    N.check(N.lib.mivit_track_directed_ml(_p(pos), _p(var), _p(frames), _p(use), n_rows, _p(offsets), n, float(dt), float(blur),
                                          _p(D), _p(D_std), _p(v), _p(v_std), _p(loglik), _p(n_inc), _p(status), _s(pos)),
            "mivit_track_directed_ml")
    return D, D_std, v, v_std, loglik, n_inc, status


def track_directed_loglik(pos: torch.Tensor, offsets: torch.Tensor, D: torch.Tensor, velocity=None, var=None, frames=None,
                          use=None, dt: float = 1.0, blur: float = 0.0):
    """The exact log-likelihood of every row range under directed motion at given parameters (csrc/directed_ml.hip,
    mivit_track_directed_loglik): pos, offsets, var, frames, use, dt, blur as track_diffusion_ml; D [n] float64 the diffusion
    coefficient of every range; velocity [n, 2] float64 (y, x), or None for the velocity that maximises the likelihood ->
    loglik [n] float64 with a velocity given, (loglik, velocity [n, 2], velocity_std [n, 2]) with None.  loglik is NaN without
    an increment and where D is negative or not finite or a given velocity is not finite, -inf for a rejected candidate.  See
    include/mivit_hip.h for the arithmetic and helpers/msd.directed_loglik for the front end."""
    name = "track_directed_loglik"
    pos, offsets, var, frames, use, n_rows, n = _track_ml_args(name, pos, offsets, var, frames, use, dt,
                                                               _directed_ml_check(name, blur))
    D = _seg_tensor(D, torch.float64, 1, name, "D [n]")
    if D.numel() != n or D.device != pos.device:
        raise ValueError(f"{name}: D must be [{n}] on the device of pos, got {tuple(D.shape)}")
    if velocity is not None:
        velocity = _seg_tensor(velocity, torch.float64, 2, name, "velocity [n, 2]")
        if tuple(velocity.shape) != (n, 2) or velocity.device != pos.device:
            raise ValueError(f"{name}: velocity must be [{n}, 2] on the device of pos, got {tuple(velocity.shape)}")
    loglik = torch.empty(n, dtype=torch.float64, device=pos.device)
    v_hat, v_hat_std = (None, None) if velocity is not None else (torch.empty(n, 2, dtype=torch.float64, device=pos.device)
                                                                  for _ in range(2))
    N.check(N.lib.mivit_track_directed_loglik(_p(pos), _p(var), _p(frames), _p(use), n_rows, _p(offsets), n, float(dt),
                                              float(blur), _p(D), _p(velocity), _p(loglik), _p(v_hat), _p(v_hat_std), _s(pos)),
            "mivit_track_directed_loglik")
    return loglik if velocity is not None else (loglik, v_hat, v_hat_std)


DRIFT_MAX_PAIRS = 4096      # csrc/drift.hip: increments of one frame that the median sorts in LDS (8 B a pair, 32 KiB)
DRIFT_MODES = {"mean": 0, "median": 1}


def drift_frames(pos: torch.Tensor, pair_row: torch.Tensor, frame_offsets: torch.Tensor, mode="mean") -> torch.Tensor:
    """The mean or the exact median of the increments of every frame (csrc/drift.hip, mivit_drift_frames): pos [N, 2] float64
    on the GPU, the table sorted by track; pair_row [M] int32 in [1, N): increment m is pos[r] - pos[r - 1] with r =
    pair_row[m]; frame_offsets [F + 1] int32, the CSR of pair_row over the frames (from 0 to M); mode "mean" (0) or "median"
    (1) -> stat [F, 2] float64, 0 for a frame without a pair.  The median sorts a frame in LDS: at most DRIFT_MAX_PAIRS pairs a
    frame.  frame_offsets and the range of pair_row are read back to be checked: every rejection is a ValueError before any
    launch.  See include/mivit_hip.h for the summation order and helpers/msd.estimate_drift for the front end."""
    pos = _seg_tensor(pos, torch.float64, 2, "drift_frames", "pos [N, 2]")
    pair_row = _seg_tensor(pair_row, torch.int32, 1, "drift_frames", "pair_row [M]")
    frame_offsets = _seg_tensor(frame_offsets, torch.int32, 1, "drift_frames", "frame_offsets [F + 1]")
    if pos.shape[1] != 2:
        raise ValueError(f"drift_frames: pos must be [N, 2], got {tuple(pos.shape)}")
    if frame_offsets.numel() < 1:
        raise ValueError("drift_frames: frame_offsets must have F + 1 entries")
    if isinstance(mode, bool) or mode not in DRIFT_MODES and mode not in DRIFT_MODES.values():
        raise ValueError(f"drift_frames: mode must be 'mean' (0) or 'median' (1), got {mode!r}")
    mode = DRIFT_MODES.get(mode, mode)
    if len({t.device for t in (pos, pair_row, frame_offsets)}) != 1:
        raise ValueError("drift_frames: all tensors must be on one device")
    n, M, F = pos.shape[0], pair_row.numel(), frame_offsets.numel() - 1
    off = frame_offsets.cpu()
    if int(off[0]) != 0 or int(off[-1]) != M or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"drift_frames: frame_offsets must rise from 0 to the number of pairs {M}")
    max_pairs = int((off[1:] - off[:-1]).max()) if F else 0
    if mode == 1 and max_pairs > DRIFT_MAX_PAIRS:
        raise ValueError(f"drift_frames: a frame of {max_pairs} pairs, the median's limit is {DRIFT_MAX_PAIRS} (DRIFT_MAX_PAIRS)")
    if M and (int(pair_row.min()) < 1 or int(pair_row.max()) >= n):
        raise ValueError(f"drift_frames: pair_row must lie in [1, {n}), the later row of an increment")
    stat = torch.empty(F, 2, dtype=torch.float64, device=pos.device)
    N.check(N.lib.mivit_drift_frames(_p(pos), n, _p(pair_row), M, _p(frame_offsets), F, mode, max_pairs, _p(stat), _s(pos)),
            "mivit_drift_frames")
    return stat


def drift_integrate(stat: torch.Tensor, n_pairs: torch.Tensor, half_window: int = 0):
    """The windowed velocity and its running sum (csrc/drift.hip, mivit_drift_integrate): stat [F, 2] float64 and n_pairs [F]
    int32 on the GPU, half_window h >= 0 -> (velocity [F, 2], drift [F, 2]) float64.  velocity[f] is the mean of stat over the
    frames max(1, f - h) .. min(F - 1, f + h) weighted by n_pairs (stat[f] itself for h = 0), velocity[0] = 0, and drift its
    running sum in blocks of 256 frames.  See include/mivit_hip.h for the order."""
    stat = _seg_tensor(stat, torch.float64, 2, "drift_integrate", "stat [F, 2]")
    n_pairs = _seg_tensor(n_pairs, torch.int32, 1, "drift_integrate", "n_pairs [F]")
    if stat.shape[1] != 2 or n_pairs.numel() != stat.shape[0]:
        raise ValueError(f"drift_integrate: stat must be [F, 2] and n_pairs [F], got {tuple(stat.shape)} and {tuple(n_pairs.shape)}")
    if stat.device != n_pairs.device:
        raise ValueError("drift_integrate: all tensors must be on one device")
    if isinstance(half_window, bool) or int(half_window) != half_window or half_window < 0:
        raise ValueError(f"drift_integrate: half_window must be an integer >= 0, got {half_window}")
    F = stat.shape[0]
    velocity, drift = torch.empty_like(stat), torch.empty_like(stat)
    N.check(N.lib.mivit_drift_integrate(_p(stat), _p(n_pairs), F, min(int(half_window), 2 ** 31 - 1), _p(velocity), _p(drift),
                                        _s(stat)), "mivit_drift_integrate")
    return velocity, drift


MOVIE_MAX_RADIUS = 64        # csrc/movie.hip: limits of mivit_render_movie
MOVIE_MAX_NPOS = 256
MOVIE_MAX_UP = 64
MOVIE_PARTICLE_CHUNK = 256   # (particle, sub-position) pairs the kernel culls per pass


def render_movie(pos: torch.Tensor, amp: torch.Tensor, sigma_hr: float, up: int, radius: int, H: int, W: int, first=None,
                 last=None) -> torch.Tensor:
    """Noise-free movie of a whole field of view (csrc/movie.hip, mivit_render_movie): pos [Np, F * npos, 2] float32 (y, x) in
    camera pixels, amp [Np, F, npos] float32, first / last [Np] int32 or both None (frames first .. last inclusive), all on the
    GPU -> movie [F, H, W] float32.  See include/mivit_hip.h for the image model and helpers/generation.render_movie for the
    float64 restatement."""
    pos = _dev_tensor(pos, torch.float32, 3, "render_movie", "pos [Np, F * npos, 2]")
    amp = _dev_tensor(amp, torch.float32, 3, "render_movie", "amp [Np, F, npos]")
    Np, F, npos = amp.shape
    if tuple(pos.shape) != (Np, F * npos, 2):
        raise ValueError(f"render_movie: pos must be [{Np}, {F * npos}, 2] for amp {tuple(amp.shape)}, got {tuple(pos.shape)}")
    if (first is None) != (last is None):
        raise ValueError("render_movie: first and last must both be given or both be None")
    if first is not None:
        first = _dev_tensor(first, torch.int32, 1, "render_movie", "first [Np]")
        last = _dev_tensor(last, torch.int32, 1, "render_movie", "last [Np]")
        if first.numel() != Np or last.numel() != Np:
            raise ValueError(f"render_movie: first and last must be [{Np}]")
    movie = torch.empty(F, int(H), int(W), dtype=torch.float32, device=amp.device)
    N.check(N.lib.mivit_render_movie(_p(pos), _p(amp), _p(first), _p(last), Np, F, npos, float(sigma_hr), int(up), int(radius),
                                     int(H), int(W), _p(movie), _s(movie)), "mivit_render_movie")
    return movie


TRANSPORT_CLASSES = {"both": 0, "directed": 1, "diffusive": 2}


def segment_transport(pos: torch.Tensor, offsets: torch.Tensor, min_len: int = 4, penalty: float = 3.0,
                      velocity_penalty: float = 3.0, min_var: float = 1e-12, classes: str = "both"):
    """The optimal partition of every track into stretches that are each diffusive (class 0) or directed (class 1: one variance
    about a constant velocity) (csrc/segment.hip, mivit_segment_transport): pos [N, 2] float64 on the GPU, sorted by track and
    by frame; offsets [n_tracks + 1] int32 (CSR, from 0 to N); classes "both", "directed" (every stretch has a velocity) or
    "diffusive" (none has: ops.segment_tracks bit for bit) -> (seg_start [N] int32, 1 on the first row of every stretch;
    seg_class [N] int32, the class of the stretch each row belongs to; cost [n_tracks] float64, NaN for a track without an
    increment).  A track has at most TRANSPORT_MAX_LEN rows.  The longest track is read back (one number) to size the kernel's
    LDS.  See include/mivit_hip.h for the recurrence and helpers/msd.segment_transport for the front end."""
    if not float(velocity_penalty) >= 0.0:
        raise ValueError(f"segment_transport: velocity_penalty must be >= 0, got {velocity_penalty}")
    if not isinstance(classes, str) or classes not in TRANSPORT_CLASSES:
        raise ValueError(f"segment_transport: classes must be one of {', '.join(TRANSPORT_CLASSES)}, got {classes!r}")
    n, n_tracks, max_len = _partition_args("segment_transport", "TRANSPORT_MAX_LEN", pos, offsets, min_len, penalty, min_var)
    seg_start = torch.zeros(n, dtype=torch.int32, device=pos.device)
    seg_class = torch.zeros(n, dtype=torch.int32, device=pos.device)
    cost = torch.empty(n_tracks, dtype=torch.float64, device=pos.device)
    if n_tracks == 0:
        return seg_start, seg_class, cost
    N.check(N.lib.mivit_segment_transport(_p(pos), n, _p(offsets), n_tracks, max_len, int(min_len), float(penalty),
                                          float(velocity_penalty), float(min_var), TRANSPORT_CLASSES[classes], _p(seg_start),
                                          _p(seg_class), _p(cost), _s(pos)), "mivit_segment_transport")
    return seg_start, seg_class, cost


def transport_stats(pos: torch.Tensor, seg_offsets: torch.Tensor, seg_track_end: torch.Tensor, dt: float = 1.0, blur: float = 0.0):
    """One row of estimates per stretch about the stretch's own velocity (csrc/segment.hip, mivit_transport_stats): pos,
    seg_offsets, seg_track_end and blur as segment_stats takes them -> (velocity [n_seg, 2] float64 (y, x) per unit of dt,
    D_res, D_cve, sigma2 [n_seg] float64, n_increments [n_seg] int32).  See include/mivit_hip.h for the arithmetic."""
    n_seg = _stretch_stats_args("transport_stats", pos, seg_offsets, seg_track_end, dt, blur)
    velocity = torch.empty(n_seg, 2, dtype=torch.float64, device=pos.device)
    d_res, d_cve, sigma2 = (torch.empty(n_seg, dtype=torch.float64, device=pos.device) for _ in range(3))
    n_inc = torch.empty(n_seg, dtype=torch.int32, device=pos.device)
    N.check(N.lib.mivit_transport_stats(_p(pos), pos.shape[0], _p(seg_offsets), _p(seg_track_end), n_seg, float(dt), float(blur),
                                        _p(velocity), _p(d_res), _p(d_cve), _p(sigma2), _p(n_inc), _s(pos)),
            "mivit_transport_stats")
    return velocity, d_res, d_cve, sigma2, n_inc
