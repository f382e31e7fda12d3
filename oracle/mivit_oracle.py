"""CPU oracle for the MiViT hot path -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline``
leg may import this file.  Nothing under ``moleculardiffusion_mivit_amd/`` does.

It is a plain-PyTorch, fp32 (or fp64), functional restatement of the arithmetic
the reference executes in ``helpers/models.py`` (reference = /root/reference,
Biomedical-Imaging-Group/MolecularDiffusion_MiViT).  Parameters live in a flat
``{reference state-dict key: tensor}`` dict, so reference checkpoints load
unchanged.  Every function cites the reference lines it restates.

Parity status: PINNED.  ``tests/golden/make_golden.py`` imported the real
reference in the build container, copied identical weights into both, and
checked outputs / loss / every parameter gradient (see tests/golden/README.md);
the committed ``tests/golden/*.npz`` vectors were produced by the reference
itself and ``tests/test_oracle_golden.py`` re-checks this file against them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, asdict
from typing import Dict, Optional

import torch
import torch.nn.functional as F

MAX_TOKENS = 128  # helpers/models.py:8 -- length of the learned positional table


@dataclass
class MiViTConfig:
    """Constructor surface of ``GeneralTransformer`` (helpers/models.py:279-294)."""
    embedding: str = "linear"          # 'linear' | 'cnn' | 'deepresnet'  (models.py:146,170,230)
    patch_size: int = 9
    embed_dim: int = 64
    num_heads: int = 4
    hidden_dim: int = 128
    num_layers: int = 6
    activation: str = "relu"           # tr_activation_fct: relu | leaky_relu | gelu
    use_pos_encoding: bool = False
    use_regression_token: bool = True
    use_global_features: bool = False
    fusion_type: str = "early"         # 'early' | 'late'
    global_feature_dim: Optional[int] = None
    head_hidden: int = 128             # MLPHead hidden_dim default (models.py:263)
    output_dim: int = 1

    def to_dict(self):
        return asdict(self)


_ACTS = {
    "relu": F.relu,
    "leaky_relu": F.leaky_relu,        # default negative_slope 0.01
    "gelu": F.gelu,                    # exact erf form (torch default)
}


# ----------------------------------------------------------------------------------------------
# parameter inventory (reference state-dict schema)
# ----------------------------------------------------------------------------------------------
def param_shapes(cfg: MiViTConfig) -> Dict[str, tuple]:
    """Name -> shape of every *trainable* tensor, in reference ``state_dict()`` order."""
    E, P, Fh = cfg.embed_dim, cfg.patch_size, cfg.hidden_dim
    out: Dict[str, tuple] = {}
    if cfg.use_regression_token:
        out["reg_token"] = (1, 1, E)                                   # models.py:308
    if cfg.embedding == "linear":
        out["embedding.proj.weight"] = (E, P * P)                      # models.py:151
        out["embedding.proj.bias"] = (E,)
    elif cfg.embedding == "cnn":
        out["embedding.conv.weight"] = (E, 1, P, P)                    # models.py:177
        out["embedding.conv.bias"] = (E,)
    elif cfg.embedding == "deepresnet":
        out["embedding.initial_conv.weight"] = (32, 1, 3, 3)           # models.py:233
        out["embedding.bn1.weight"] = (32,)
        out["embedding.bn1.bias"] = (32,)
        for blk, (ci, co) in (("res_block1", (32, 64)), ("res_block2", (64, 128))):  # :237-238
            out[f"embedding.{blk}.conv1.weight"] = (co, ci, 3, 3)
            out[f"embedding.{blk}.bn1.weight"] = (co,)
            out[f"embedding.{blk}.bn1.bias"] = (co,)
            out[f"embedding.{blk}.conv2.weight"] = (co, co, 3, 3)
            out[f"embedding.{blk}.bn2.weight"] = (co,)
            out[f"embedding.{blk}.bn2.bias"] = (co,)
            out[f"embedding.{blk}.skip.0.weight"] = (co, ci, 1, 1)
            out[f"embedding.{blk}.skip.1.weight"] = (co,)
            out[f"embedding.{blk}.skip.1.bias"] = (co,)
        out["embedding.fc.weight"] = (E, 128)                          # models.py:241
        out["embedding.fc.bias"] = (E,)
    else:
        raise ValueError(cfg.embedding)
    out["norm.weight"] = (E,)                                          # models.py:301
    out["norm.bias"] = (E,)
    if cfg.use_pos_encoding:
        out["transformer.pos_embedding"] = (1, MAX_TOKENS, E)          # models.py:120
    for i in range(cfg.num_layers):
        pre = f"transformer.encoder_layers.{i}."
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):          # models.py:20-23
            out[pre + f"self_attn.{nm}.weight"] = (E, E)
            out[pre + f"self_attn.{nm}.bias"] = (E,)
        out[pre + "norm1.weight"] = (E,)
        out[pre + "norm1.bias"] = (E,)
        out[pre + "norm2.weight"] = (E,)
        out[pre + "norm2.bias"] = (E,)
        out[pre + "feed_forward.fc1.weight"] = (Fh, E)                 # models.py:64-65
        out[pre + "feed_forward.fc1.bias"] = (Fh,)
        out[pre + "feed_forward.fc2.weight"] = (E, Fh)
        out[pre + "feed_forward.fc2.bias"] = (E,)
    out["transformer.norm.weight"] = (E,)                              # models.py:134
    out["transformer.norm.bias"] = (E,)
    if cfg.use_global_features:
        G = cfg.global_feature_dim
        assert G is not None, "Must provide global_feature_dim if using global features"
        out["feature_projector.0.weight"] = (E, G)                     # models.py:316-320
        out["feature_projector.0.bias"] = (E,)
        out["feature_projector.2.weight"] = (E, E)
        out["feature_projector.2.bias"] = (E,)
    head_in = 2 * E if (cfg.use_global_features and cfg.fusion_type == "late") else E  # :323-326
    out["mlp_head.mlp.0.weight"] = (cfg.head_hidden, head_in)          # models.py:268-273
    out["mlp_head.mlp.0.bias"] = (cfg.head_hidden,)
    out["mlp_head.mlp.3.weight"] = (cfg.output_dim, cfg.head_hidden)
    out["mlp_head.mlp.3.bias"] = (cfg.output_dim,)
    return out


def bn_buffer_shapes(cfg: MiViTConfig) -> Dict[str, tuple]:
    """BatchNorm running statistics of DeepResNetEmbedding (non-trainable buffers)."""
    if cfg.embedding != "deepresnet":
        return {}
    out = {}
    bns = [("embedding.bn1", 32)]
    for blk, co in (("res_block1", 64), ("res_block2", 128)):
        bns += [(f"embedding.{blk}.bn1", co), (f"embedding.{blk}.bn2", co), (f"embedding.{blk}.skip.1", co)]
    for nm, c in bns:
        out[nm + ".running_mean"] = (c,)
        out[nm + ".running_var"] = (c,)
    return out


def _hash_uniform(n: int, salt: int) -> torch.Tensor:
    """Exact-integer hash -> uniform(-1,1) float64; platform independent (no libm, no RNG stream)."""
    M = (1 << 32) - 1
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + (salt + 1) * 40503) & M
    h = ((h ^ (h >> 15)) * 2246822519) & M
    h = ((h ^ (h >> 13)) * 3266489917) & M
    h = (h ^ (h >> 16)) & M
    return h.to(torch.float64) / float(1 << 31) - 1.0


def closed_form_params(cfg: MiViTConfig, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """RNG-free deterministic weights from an integer hash (full-rank, reproducible anywhere).

    Used by golden fixtures so the vectors need not store weights and do not depend on
    torch's RNG stream.  Scales are chosen so activations stay O(1) through the stack.
    """
    params: Dict[str, torch.Tensor] = {}
    for k, (name, shape) in enumerate(param_shapes(cfg).items()):
        n = int(math.prod(shape))
        base = _hash_uniform(n, k)
        leaf = name.rsplit(".", 1)[-1]
        is_norm = (".norm" in name or name.startswith("norm.") or ".bn" in name
                   or name.endswith("skip.1.weight") or name.endswith("skip.1.bias"))
        if is_norm and leaf == "weight":
            t = 1.0 + 0.2 * base
        elif leaf == "bias":
            t = 0.1 * base
        elif name in ("reg_token", "transformer.pos_embedding"):
            t = 0.7 * base
        else:  # dense / conv weight: uniform with std ~ 1/sqrt(fan_in)
            fan_in = int(math.prod(shape[1:])) if len(shape) > 1 else shape[0]
            t = base * (1.7 / math.sqrt(fan_in))
        params[name] = t.reshape(shape).to(dtype)
    for k, (name, shape) in enumerate(bn_buffer_shapes(cfg).items()):
        base = _hash_uniform(shape[0], 1000 + k)
        if name.endswith("running_mean"):
            params[name] = (0.05 * base).to(dtype)
        else:
            params[name] = (1.0 + 0.2 * base ** 2).to(dtype)
    return params


def random_params(cfg: MiViTConfig, seed: int = 0, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """Random weights following the reference initialisers' *distributions* (not its RNG stream)."""
    g = torch.Generator().manual_seed(seed)
    params: Dict[str, torch.Tensor] = {}
    for name, shape in param_shapes(cfg).items():
        leaf = name.rsplit(".", 1)[-1]
        is_norm = (".norm" in name or name.startswith("norm.") or ".bn" in name
                   or name.endswith("skip.1.weight") or name.endswith("skip.1.bias"))
        if is_norm:
            t = torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
        elif name in ("reg_token", "transformer.pos_embedding"):
            t = torch.randn(shape, generator=g)                              # models.py:120,308
        elif "self_attn" in name and leaf == "weight":
            bound = math.sqrt(6.0 / (shape[0] + shape[1]))                   # xavier_uniform :28-31
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        else:
            fan_in = int(math.prod(shape[1:])) if len(shape) > 1 else None
            if fan_in is None:  # bias: bound uses the matching weight's fan_in
                wshape = param_shapes(cfg)[name[: -len("bias")] + "weight"]
                fan_in = int(math.prod(wshape[1:]))
            bound = 1.0 / math.sqrt(fan_in)                                  # nn.Linear / Conv default
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        params[name] = t.to(dtype)
    for name, shape in bn_buffer_shapes(cfg).items():
        params[name] = (torch.zeros(shape) if name.endswith("mean") else torch.ones(shape)).to(dtype)
    return params


# ----------------------------------------------------------------------------------------------
# the arithmetic
# ----------------------------------------------------------------------------------------------
def layer_norm(x, w, b, eps: float = 1e-5):
    """nn.LayerNorm(E) over the last dim, biased variance (models.py:88-89,134,301)."""
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) * torch.rsqrt(var + eps) * w + b


def embed_linear(x, w, b):
    """LinearProjectionEmbedding.forward (models.py:153-167): one token per whole frame."""
    if x.dim() == 3:                                   # (T,P,P) -> adds a batch dim (:154-158)
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError(f"Unexpected input shape: {tuple(x.shape)}")
    B, T, h, wd = x.shape
    assert h == wd and h * wd == w.shape[1], "Patch size mismatch"
    return F.linear(x.reshape(B, T, h * wd), w, b)


def embed_cnn(x, w, b):
    """CNNEmbedding.forward (models.py:179-199): Conv2d(1,E,kernel=P) == linear embed, W viewed (E,1,P,P)."""
    B, T, h, wd = x.shape
    assert h == wd == w.shape[-1], "Patch size mismatch"
    return F.linear(x.reshape(B, T, h * wd), w.reshape(w.shape[0], -1), b)


def _bn(x, p, pre, training, momentum=0.1, eps=1e-5, stats_out=None):
    rm, rv = p[pre + ".running_mean"], p[pre + ".running_var"]
    if training:
        # batch statistics over (N,H,W); running buffers get the unbiased variance (torch semantics)
        y = F.batch_norm(x, None, None, p[pre + ".weight"], p[pre + ".bias"], True, momentum, eps)
        if stats_out is not None:
            n = x.numel() / x.shape[1]
            m = x.mean(dim=(0, 2, 3))
            v = x.var(dim=(0, 2, 3), unbiased=False)
            stats_out[pre + ".running_mean"] = (1 - momentum) * rm + momentum * m
            stats_out[pre + ".running_var"] = (1 - momentum) * rv + momentum * v * n / max(n - 1, 1)
        return y
    return F.batch_norm(x, rm, rv, p[pre + ".weight"], p[pre + ".bias"], False, momentum, eps)


def _res_block(x, p, pre, training, stats_out):
    """ResidualBlock.forward (models.py:220-228), projection skip, no down-sampling."""
    idt = F.conv2d(x, p[pre + ".skip.0.weight"])
    idt = _bn(idt, p, pre + ".skip.1", training, stats_out=stats_out)
    out = F.conv2d(x, p[pre + ".conv1.weight"], padding=1)
    out = F.relu(_bn(out, p, pre + ".bn1", training, stats_out=stats_out))
    out = F.conv2d(out, p[pre + ".conv2.weight"], padding=1)
    out = _bn(out, p, pre + ".bn2", training, stats_out=stats_out)
    return F.relu(out + idt)


def embed_deepresnet(x, p, training=True, stats_out=None):
    """DeepResNetEmbedding.forward (models.py:243-257)."""
    B, T, h, w = x.shape
    y = x.reshape(B * T, 1, h, w)
    y = F.conv2d(y, p["embedding.initial_conv.weight"], padding=1)
    y = F.relu(_bn(y, p, "embedding.bn1", training, stats_out=stats_out))
    y = _res_block(y, p, "embedding.res_block1", training, stats_out)
    y = _res_block(y, p, "embedding.res_block2", training, stats_out)
    y = y.mean(dim=(2, 3)).reshape(B, T, 128)
    return F.linear(y, p["embedding.fc.weight"], p["embedding.fc.bias"])


def attention(x, p, pre, H, trace=None):
    """MultiHeadAttention.forward (models.py:33-59), mask=None, dropout p=0."""
    B, S, E = x.shape
    Dh = E // H
    assert Dh * H == E, "embed_dim must be divisible by num_heads"

    def proj(nm):
        y = F.linear(x, p[pre + nm + ".weight"], p[pre + nm + ".bias"])
        return y.reshape(B, S, H, Dh).permute(0, 2, 1, 3)                      # [B,H,S,Dh]
    q, k, v = proj("q_proj"), proj("k_proj"), proj("v_proj")
    scores = (q @ k.transpose(-1, -2)) / math.sqrt(Dh)                         # :42
    attn = torch.softmax(scores, dim=-1)                                       # :47
    ctx = (attn @ v).permute(0, 2, 1, 3).reshape(B, S, E)                      # :51-54
    out = F.linear(ctx, p[pre + "out_proj.weight"], p[pre + "out_proj.bias"])     # :57
    if trace is not None:
        trace.update(q=q, k=k, v=v, attn=attn, ctx=ctx, attn_out=out)
    return out


def encoder_layer(x, p, pre, H, act, trace=None):
    """TransformerEncoderLayerWithSkip.forward (models.py:97-108): post-norm residual wiring."""
    a = attention(x, p, pre + "self_attn.", H, trace)
    z1 = x + a
    x1 = layer_norm(z1, p[pre + "norm1.weight"], p[pre + "norm1.bias"])        # :100-101
    u = F.linear(x1, p[pre + "feed_forward.fc1.weight"], p[pre + "feed_forward.fc1.bias"])
    h = act(u)                                                                  # :73-74
    f = F.linear(h, p[pre + "feed_forward.fc2.weight"], p[pre + "feed_forward.fc2.bias"])
    z2 = x1 + f
    x2 = layer_norm(z2, p[pre + "norm2.weight"], p[pre + "norm2.bias"])        # :105-106
    if trace is not None:
        trace.update(z1=z1, x1=x1, u=u, h=h, ffn=f, z2=z2, x2=x2)
    return x2


def embed(p: Dict[str, torch.Tensor], cfg: MiViTConfig, x, training=True, bn_stats_out: Optional[dict] = None):
    """The embedding step of GeneralTransformer.forward (models.py:331): frames [B,T,P,P] -> pre-norm tokens [B,T,E]."""
    if cfg.embedding == "linear":
        return embed_linear(x, p["embedding.proj.weight"], p["embedding.proj.bias"])
    if cfg.embedding == "cnn":
        return embed_cnn(x, p["embedding.conv.weight"], p["embedding.conv.bias"])
    return embed_deepresnet(x, p, training, bn_stats_out)


def forward(p: Dict[str, torch.Tensor], cfg: MiViTConfig, x, features=None, training=True,
            trace: Optional[dict] = None, bn_stats_out: Optional[dict] = None):
    """GeneralTransformer.forward (models.py:328-361) + Transformer.forward (:136-141)."""
    return forward_from_tokens(p, cfg, embed(p, cfg, x, training, bn_stats_out), features, trace)


def forward_from_tokens(p: Dict[str, torch.Tensor], cfg: MiViTConfig, tok, features=None, trace: Optional[dict] = None):
    """Everything behind the embedding (models.py:334-361): the trunk on pre-norm tokens [B,T,E].  No ``embedding.*``
    parameter is read, so autograd through ``tok`` gives the d(tokens) an external embedding receives."""
    act = _ACTS[cfg.activation]
    tok_n = layer_norm(tok, p["norm.weight"], p["norm.bias"])                  # :334
    B = tok_n.shape[0]

    def project_features():
        assert features is not None, "Global features required"
        hid_pre = F.linear(features, p["feature_projector.0.weight"], p["feature_projector.0.bias"])
        if trace is not None:
            trace["fp_pre"] = hid_pre
        return F.linear(F.relu(hid_pre), p["feature_projector.2.weight"], p["feature_projector.2.bias"])

    seq = tok_n
    if cfg.use_regression_token:                                               # :338-347
        reg = p["reg_token"].expand(B, 1, -1)
        if cfg.use_global_features and cfg.fusion_type == "early":
            reg = reg + project_features().unsqueeze(1)
        seq = torch.cat([reg, tok_n], dim=1)
    if cfg.use_pos_encoding:                                                   # :137-138
        seq = seq + p["transformer.pos_embedding"][:, : seq.shape[1], :]
    if trace is not None:
        trace.update(embed=tok, embed_ln=tok_n, x0=seq, layers=[])
    for i in range(cfg.num_layers):                                            # :139-140
        lt = {} if trace is not None else None
        seq = encoder_layer(seq, p, f"transformer.encoder_layers.{i}.", cfg.num_heads, act, lt)
        if trace is not None:
            trace["layers"].append(lt)
    seq = layer_norm(seq, p["transformer.norm.weight"], p["transformer.norm.bias"])  # :141
    pooled = seq[:, 0, :] if cfg.use_regression_token else seq.mean(dim=1)     # :351-354
    if cfg.use_global_features and cfg.fusion_type == "late":                  # :356-359
        pooled = torch.cat([pooled, project_features()], dim=-1)
    head_pre = F.linear(pooled, p["mlp_head.mlp.0.weight"], p["mlp_head.mlp.0.bias"])         # :268-273
    out = F.linear(F.relu(head_pre), p["mlp_head.mlp.3.weight"], p["mlp_head.mlp.3.bias"])
    if trace is not None:
        trace.update(final=seq, pooled=pooled, head_pre=head_pre, out=out)
    return out


def loss_and_grads(p, cfg, x, labels, features=None, training=True):
    """MSELoss(mean) + autograd gradients (trainSettingsPSFNoise.py:31, trainModelsPSFNoise.py:191-192)."""
    leaves = {k: v.detach().clone().requires_grad_(k in param_shapes(cfg)) for k, v in p.items()}
    out = forward(leaves, cfg, x, features, training)
    loss = F.mse_loss(out, labels)
    names = [k for k in param_shapes(cfg)]
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return out.detach(), loss.detach(), dict(zip(names, grads))


class OracleModule(torch.nn.Module):
    """nn.Module shell around the functional oracle so stock optimizers can drive it
    (used as the timed 'port' CPU baseline in bench.py and in training-trajectory tests)."""

    def __init__(self, cfg: MiViTConfig, params: Optional[Dict[str, torch.Tensor]] = None, seed: int = 0):
        super().__init__()
        self.cfg = cfg
        params = params if params is not None else random_params(cfg, seed)
        self._names = list(param_shapes(cfg))
        self._pl = torch.nn.ParameterList([torch.nn.Parameter(params[k].clone()) for k in self._names])
        self._bufnames = list(bn_buffer_shapes(cfg))
        for k in self._bufnames:
            self.register_buffer(k.replace(".", "__"), params[k].clone())

    def ref_state_dict(self) -> Dict[str, torch.Tensor]:
        d = {k: v for k, v in zip(self._names, self._pl)}
        for k in self._bufnames:
            d[k] = getattr(self, k.replace(".", "__"))
        return d

    def forward(self, x, features=None):
        p = self.ref_state_dict()
        stats = {} if (self.training and self._bufnames) else None
        out = forward(p, self.cfg, x, features, training=self.training, bn_stats_out=stats)
        if stats:
            with torch.no_grad():
                for k, v in stats.items():
                    getattr(self, k.replace(".", "__")).copy_(v)
        return out


# ----------------------------------------------------------------------------------------------
# synthetic input: background N(0.2,0.06^2) + jittered Gaussian PSF blob, label D/10
# ----------------------------------------------------------------------------------------------
def synthetic_batch(B, T, P, seed=1234, features_dim=None, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    D = torch.rand(B, generator=g) * 9.9 + 0.1
    steps = torch.randn(B, T, 2, generator=g) * torch.sqrt(2 * D * 0.01).view(B, 1, 1) * (P / 9.0)
    pos = torch.cumsum(steps, dim=1)
    pos = pos - pos.mean(dim=1, keepdim=True) + (P - 1) / 2.0
    yy = torch.arange(P, dtype=torch.float32).view(1, 1, P, 1)
    xx = torch.arange(P, dtype=torch.float32).view(1, 1, 1, P)
    sig = 1.1 * P / 9.0
    blob = torch.exp(-((yy - pos[..., 1].view(B, T, 1, 1)) ** 2 + (xx - pos[..., 0].view(B, T, 1, 1)) ** 2)
                     / (2 * sig * sig))
    x = 0.2 + 0.06 * torch.randn(B, T, P, P, generator=g) + 0.6 * blob
    labels = (D / 10.0).view(B, 1)
    feats = torch.randn(B, features_dim, generator=g) if features_dim else None
    return (x.float().to(device), labels.float().to(device),
            feats.float().to(device) if feats is not None else None)


def closed_form_batch(B, T, P, features_dim=None, dtype=torch.float32, salt=0):
    """RNG-free input used by the golden fixtures: background ripple + a wandering Gaussian blob.

    Mimics the value range of ``normalize_images`` output (helpersGeneration.py:356-400):
    roughly -0.05 .. 0.9, blob near the frame centre.  Labels are D/10 in (0,1].
    """
    b = torch.arange(B, dtype=torch.float64).view(B, 1, 1, 1)
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1, 1)
    i = torch.arange(P, dtype=torch.float64).view(1, 1, P, 1)
    j = torch.arange(P, dtype=torch.float64).view(1, 1, 1, P)
    c = (P - 1) / 2.0
    amp = 0.15 * P / 9.0 * (1.0 + 0.5 * b)
    cy = c + amp * torch.sin(0.9 * t + 0.7 * b)
    cx = c + amp * torch.cos(0.6 * t + 1.1 * b + 0.3)
    sig = 1.1 * P / 9.0
    blob = torch.exp(-((i - cy) ** 2 + (j - cx) ** 2) / (2 * sig * sig))
    noise = _hash_uniform(B * T * P * P, 7777 + 31 * salt).view(B, T, P, P) * (0.06 * math.sqrt(3.0))
    x = 0.2 + noise + (0.35 + 0.3 * torch.sin(1.3 * b + 0.21 * t) ** 2) * blob
    labels = (0.05 + 0.9 * (torch.arange(B, dtype=torch.float64) + 0.5) / B).view(B, 1)
    feats = None
    if features_dim:
        fb = torch.arange(B, dtype=torch.float64).view(B, 1)
        ff = torch.arange(features_dim, dtype=torch.float64).view(1, features_dim)
        feats = (1.5 * _hash_uniform(B * features_dim, 8888 + 31 * salt).view(B, features_dim)).to(dtype)
    return x.to(dtype), labels.to(dtype), feats


def min_kink_margin(p, cfg, x, features=None, training=True) -> float:
    """Smallest |pre-activation| at any ReLU / leaky-ReLU site, evaluated in fp64.

    Two correct fp32 implementations can disagree about the sign of a pre-activation that is within
    rounding noise of zero, which flips one ReLU mask bit and moves individual weight gradients by
    ~1e-3 relative.  Golden inputs are chosen (salt search in make_golden.py) so this margin stays
    far above fp32 noise, making gradient comparisons at 1e-4 meaningful.
    """
    p64 = {k: v.double() for k, v in p.items()}
    tr = {}
    forward(p64, cfg, x.double(), None if features is None else features.double(), training=training, trace=tr)
    m = float(tr["head_pre"].abs().min())
    if "fp_pre" in tr:
        m = min(m, float(tr["fp_pre"].abs().min()))
    if cfg.activation in ("relu", "leaky_relu"):
        for lt in tr["layers"]:
            m = min(m, float(lt["u"].abs().min()))
    return m
