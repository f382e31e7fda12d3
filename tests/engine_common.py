"""Case table, fp64 reference, bf16-autocast yardstick and arena packing of the engine-dispatch suites
(tests/test_engine_paths.py on the host, tests/test_engine_paths_gpu.py on the device).  Host only: nothing here imports the
HIP library, so the table and both oracles are checked where no GPU exists.  At the end: `Rig` and `Guarded`, the device
buffers of tests/test_engine_paths_gpu.py and tests/test_graph_replay_gpu.py; they load the library when one is made.

A case is one point of the constructor surface chosen for the BRANCH of csrc/engine.hip it reaches (fused blocks or per-operator
layers, the stage-0 readout variants, the zero-layer trunk, the external embedding), not for the experiment it mirrors; the
shapes are the smallest that reach the branch."""
import functools
from dataclasses import dataclass
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import mivit_oracle as orc

FP32_TOL = 1e-4            # BASELINE.json north_star
KINK_MARGIN = 4e-6         # tests/golden/make_golden.py: smallest |pre-activation| at any ReLU site, in fp64
PATCH = 9                  # 81 pixels per frame row: an odd leading dimension
SENTINEL = 0x7FC0BEEF      # a quiet NaN with a recognisable payload (tests/gpu_buffers.py uses the same word)
PRECISIONS = ("fp32", "bf16", "fp16")
# 16-bit floors of test_bf16_as_accurate_as_torch_autocast: error <= 3 x yardstick + floor
LOWP_FLOOR = {"out": 2e-2, "loss": 3e-2, "grad": 5e-2}


@dataclass(frozen=True)
class Case:
    name: str
    cfg: orc.MiViTConfig       # for `external` the oracle config is a linear one whose embedding.* parameters the trunk never reads
    T: int
    embedding: str             # 'linear' | 'cnn' | 'external'
    path: str                  # layers of the 16-bit precisions: 'fused' | 'per_operator' | 'none' (no layer); fp32 never fuses
    dfeatures: bool = False
    dx_tokens: bool = False
    fp32_B1: bool = False      # fp32 additionally runs a single sequence

    @property
    def S(self):
        return self.T + (1 if self.cfg.use_regression_token else 0)

    @property
    def fusion(self):
        return self.cfg.fusion_type if self.cfg.use_global_features else "none"

    def batches(self, precision):
        """fp32: 3 sequences (and 1 where the table says so); 16-bit: 24, so that one ReLU flip in the head does not move
        every upstream gradient by ~15 % (comment in test_bf16_as_accurate_as_torch_autocast)."""
        if precision == "fp32":
            return (3, 1) if self.fp32_B1 else (3,)
        return (24,)


def _cfg(E, H, Fh, L, act="relu", **kw):
    emb = kw.pop("embedding", "linear")
    return orc.MiViTConfig(embedding=emb, patch_size=PATCH, embed_dim=E, num_heads=H, hidden_dim=Fh, num_layers=L,
                           activation=act, **kw)


_MEAN = dict(use_regression_token=False)
# At 24 sequences T = 11 / 12 / 13 / 20 / 63 / 64 give >= 256 frame rows (the small-frame embedding kernels engage), T <= 7 do not.
CASES = [
    Case("w64_fused_S12", _cfg(64, 4, 128, 2), 11, "linear", "fused"),
    Case("w64_fused_S64", _cfg(64, 4, 128, 2), 63, "linear", "fused"),
    Case("w64_perop_S65", _cfg(64, 4, 128, 2), 64, "linear", "per_operator"),
    Case("w128_gelu_pos_fused_S12", _cfg(128, 4, 256, 2, "gelu", use_pos_encoding=True), 11, "linear", "fused"),
    Case("w128_gelu_pos_perop_S65", _cfg(128, 4, 256, 2, "gelu", use_pos_encoding=True), 64, "linear", "per_operator"),
    Case("w128_leaky_early", _cfg(128, 4, 256, 1, "leaky_relu", use_global_features=True, fusion_type="early",
                                  global_feature_dim=25), 13, "linear", "fused", dfeatures=True),
    # (T = 13, not 11: at T = 11 fp32 arithmetic itself leaves 1.1e-5 of rounding noise in the analytically zero k_proj.bias
    #  gradient, more than the tenth of FP32_TOL a reference may use up -- tests/test_engine_paths.py)
    Case("w128_meanpool_late_out3", _cfg(128, 4, 256, 2, use_global_features=True, fusion_type="late", global_feature_dim=25,
                                         output_dim=3, head_hidden=36, **_MEAN), 12, "linear", "fused", dfeatures=True),
    Case("w64_meanpool_pos_S1", _cfg(64, 4, 128, 3, use_pos_encoding=True, **_MEAN), 1, "linear", "fused"),
    Case("w64_S2_B1", _cfg(64, 4, 128, 2), 1, "linear", "fused", fp32_B1=True),
    Case("w32_leaky_meanpool_pos_late", _cfg(32, 2, 64, 3, "leaky_relu", use_pos_encoding=True, use_global_features=True,
                                             fusion_type="late", global_feature_dim=7, **_MEAN), 20, "linear", "per_operator",
         dfeatures=True),
    Case("w128_heads8_gelu", _cfg(128, 8, 256, 2, "gelu"), 11, "linear", "per_operator"),
    Case("w64_hidden256", _cfg(64, 4, 256, 2), 11, "linear", "per_operator"),
    Case("w96_heads3", _cfg(96, 3, 160, 1), 5, "linear", "per_operator"),        # no streaming kernel serves this width
    Case("w256_heads8", _cfg(256, 8, 128, 1), 5, "linear", "per_operator"),
    Case("L0_early", _cfg(64, 4, 128, 0, use_global_features=True, fusion_type="early", global_feature_dim=25), 11, "linear",
         "none"),
    Case("L0_meanpool", _cfg(64, 4, 128, 0, **_MEAN), 11, "linear", "none"),
    Case("external_w64", _cfg(64, 4, 128, 2), 11, "external", "fused", dx_tokens=True),
    Case("external_w32_gelu_meanpool_late", _cfg(32, 2, 64, 2, "gelu", use_global_features=True, fusion_type="late",
                                                 global_feature_dim=7, **_MEAN), 7, "external", "per_operator", dfeatures=True,
         dx_tokens=True),
    Case("cnn_out3", _cfg(64, 4, 128, 1, embedding="cnn", output_dim=3), 11, "cnn", "fused"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
GRAPH_CASES = ("w64_perop_S65", "w128_meanpool_late_out3", "external_w32_gelu_meanpool_late")


def param_names(case):
    """The parameters the engine owns, in reference state-dict order (an external embedding's live outside it)."""
    return [k for k in orc.param_shapes(case.cfg) if not (case.embedding == "external" and k.startswith("embedding."))]


@functools.lru_cache(maxsize=None)
def _batch64(name, B, salt):
    """(frames, engine input, labels, features) in fp64.  The engine input is the frames, or for `external` the pre-norm
    tokens an fp64 linear embedding makes of them."""
    case = CASE_BY_NAME[name]
    cfg = case.cfg
    frames, labels, feats = orc.closed_form_batch(B, case.T, cfg.patch_size, cfg.global_feature_dim if cfg.use_global_features else None,
                                                  dtype=torch.float64, salt=salt)
    if cfg.output_dim > 1:
        labels = labels.repeat(1, cfg.output_dim) * torch.linspace(0.5, 1.0, cfg.output_dim, dtype=torch.float64)
    x = frames
    if case.embedding == "external":
        with torch.no_grad():
            x = orc.embed(orc.closed_form_params(cfg, dtype=torch.float64), cfg, frames)
    return frames, x, labels, feats


def batch(case, B, salt, dtype=torch.float64):
    """(engine input, labels, features) of a case in `dtype` (fp64 values rounded once)."""
    _, x, labels, feats = _batch64(case.name, B, salt)
    return x.to(dtype), labels.to(dtype), None if feats is None else feats.to(dtype)


def _run_oracle(case, B, salt, dtype, autocast):
    cfg = case.cfg
    names = param_names(case)
    leaves = {k: v.detach().clone().requires_grad_(k in names) for k, v in orc.closed_form_params(cfg, dtype=dtype).items()}
    x, labels, feats = batch(case, B, salt, dtype)
    wrt = [leaves[k] for k in names]
    if case.dfeatures:
        feats = feats.clone().requires_grad_()
        wrt.append(feats)
    if case.dx_tokens:
        x = x.clone().requires_grad_()
        wrt.append(x)

    def run():
        out = orc.forward_from_tokens(leaves, cfg, x, feats) if case.embedding == "external" else orc.forward(leaves, cfg, x, feats)
        return out, F.mse_loss(out.to(dtype), labels)

    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out, loss = run()
    else:
        out, loss = run()
    g = list(torch.autograd.grad(loss, wrt))
    res = SimpleNamespace(out=out.detach().to(dtype), loss=loss.detach(), grads={k: g[i].detach() for i, k in enumerate(names)},
                          dfeatures=None, dx_tokens=None)
    if case.dx_tokens:
        res.dx_tokens = g.pop().detach()
    if case.dfeatures:
        res.dfeatures = g.pop().detach()
    return res


@functools.lru_cache(maxsize=None)
def _reference(name, B, salt):
    return _run_oracle(CASE_BY_NAME[name], B, salt, torch.float64, False)


def reference(case, B, salt):
    """The oracle in fp64 on fp64 parameters and inputs: out, loss, every parameter gradient, d(features) / d(tokens) where the
    case requests them.  Computed once per (case, B, salt) and shared: treat it as read-only."""
    return _reference(case.name, B, salt)


@functools.lru_cache(maxsize=None)
def _yardstick(name, B, salt):
    return _run_oracle(CASE_BY_NAME[name], B, salt, torch.float32, True)


def yardstick(case, B, salt):
    """The same oracle in fp32 under torch.autocast('cpu', bfloat16): what PyTorch's own bf16 makes of the same arithmetic."""
    return _yardstick(case.name, B, salt)


def oracle_fp32(case, B, salt):
    """The oracle in plain fp32 (the arithmetic the engine's parity mode restates)."""
    return _run_oracle(case, B, salt, torch.float32, False)


@functools.lru_cache(maxsize=None)
def _pick_salt(name, B):
    case = CASE_BY_NAME[name]
    p = orc.closed_form_params(case.cfg, dtype=torch.float64)
    for salt in range(64):
        frames, _, _, feats = _batch64(name, B, salt)
        if orc.min_kink_margin(p, case.cfg, frames, feats) > KINK_MARGIN:
            return salt
    return None


def pick_salt(case, B):
    """First input salt whose ReLU / leaky-ReLU pre-activations all stay clear of zero in fp64 (None: no salt below 64)."""
    return _pick_salt(case.name, B)


def nth_salt(case, B, n, params=None):
    """The n-th (from 0) input salt below 64 that is admissible in the sense of pick_salt under `params` (fp64, reference
    keys; default: the closed-form set, so nth_salt(case, B, 0) == pick_salt(case, B)).  None: fewer than n + 1 such salts."""
    p = orc.closed_form_params(case.cfg, dtype=torch.float64) if params is None else params
    for salt in range(64):
        frames, _, _, feats = _batch64(case.name, B, salt)
        if orc.min_kink_margin(p, case.cfg, frames, feats) > KINK_MARGIN:
            if n == 0:
                return salt
            n -= 1
    return None


# ---- error measures ---------------------------------------------------------------------------------------------------------
def _tensors(r):
    """Gradient tensors of a result in one dict.  d(features) / d(tokens) live on another scale than the parameter gradients
    (they are per-sample, the others batch sums), so they do not take part in the global gradient scale: their floor is
    relative to their own size."""
    t = {k: (v, False) for k, v in r.grads.items()}
    if r.dfeatures is not None:
        t["d(features)"] = (r.dfeatures, True)
    if r.dx_tokens is not None:
        t["d(tokens)"] = (r.dx_tokens, True)
    return t


def fp32_errors(got, ref):
    """out: max |diff| / max |ref|; loss: relative; gradients as _grad_err of tests/test_model_gpu.py: per tensor
    max |diff| / (max |ref| + 1e-3 x the largest parameter gradient's max).  -> {what: error}"""
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    err = {"out": float((d(got.out) - ref.out).abs().max() / ref.out.abs().max()),
           "loss": abs(float(got.loss) - float(ref.loss)) / float(ref.loss)}
    gscale = max(float(g.abs().max()) for g in ref.grads.values())
    gt = _tensors(got)
    for k, (g, own) in _tensors(ref).items():
        floor = 1e-3 * (float(g.abs().max()) if own else gscale)
        err[k] = float((d(gt[k][0]).reshape(g.shape) - g).abs().max()) / (float(g.abs().max()) + floor)
    return err


def lowp_errors(got, ref):
    """The measures of test_bf16_as_accurate_as_torch_autocast: out against max(max |ref|, 0.25), loss relative, gradients
    norm-wise per tensor against norm(ref) + 1e-2 x the largest parameter gradient's norm.  -> {what: error}"""
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    err = {"out": float((d(got.out) - ref.out).abs().max()) / max(float(ref.out.abs().max()), 0.25),
           "loss": abs(float(got.loss) - float(ref.loss)) / float(ref.loss)}
    gscale = max(float(g.norm()) for g in ref.grads.values())
    gt = _tensors(got)
    for k, (g, own) in _tensors(ref).items():
        floor = 1e-2 * (float(g.norm()) if own else gscale)
        err[k] = float((d(gt[k][0]).reshape(g.shape) - g).norm()) / (float(g.norm()) + floor)
    return err


def lowp_floor(what):
    return LOWP_FLOOR.get(what, LOWP_FLOOR["grad"])


# ---- arena ------------------------------------------------------------------------------------------------------------------
def sentinel_arena(numel):
    return torch.full((numel,), SENTINEL, dtype=torch.int32).view(torch.float32)


def pack_arena(plan, params):
    """fp32 arena in the plan's layout (param_names / param_offsets / param_numels / arena_numel) holding the oracle
    parameters; the padding between tensors holds SENTINEL, a NaN: an operand read at a wrong offset poisons the result."""
    arena = sentinel_arena(plan.arena_numel)
    for name, off, n in zip(plan.param_names, plan.param_offsets, plan.param_numels):
        t = params[name].detach().reshape(-1)
        assert t.numel() == n, (name, t.numel(), n)
        arena[off:off + n] = t.float()
    return arena


def padding_mask(plan):
    """True where the arena holds no parameter element."""
    pad = torch.ones(plan.arena_numel, dtype=torch.bool)
    for off, n in zip(plan.param_offsets, plan.param_numels):
        pad[off:off + n] = False
    return pad


def unpack_arena(plan, arena):
    return {name: arena[off:off + n] for name, off, n in zip(plan.param_names, plan.param_offsets, plan.param_numels)}


# ---- device side: one plan with guarded buffers at fixed addresses -------------------------------------------------------------
# (the HIP library is imported when a Rig is made, not when this module is: the table and the oracles stay host-only)
def _native():
    from moleculardiffusion_mivit_amd import _native as N
    return N


LOSS_SCALE = {"fp32": 1.0, "bf16": 1.0, "fp16": 4096.0}
GUARD_BYTES = 4096


class Guarded:
    """`numel` elements of `dtype` inside a larger device allocation: 256 bytes in front of and 4 KiB behind the region hold
    a byte pattern that must survive every call."""
    PATTERN = 0xA5

    def __init__(self, numel, dtype):
        self.isz = torch.empty(0, dtype=dtype).element_size()
        self.front, self.nbytes = 256, numel * self.isz
        self.raw = torch.full((self.front + self.nbytes + GUARD_BYTES,), self.PATTERN, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        self.t = self.raw[self.front:self.front + self.nbytes].view(dtype)

    def intact(self):
        return bool((self.raw[:self.front] == self.PATTERN).all()) and bool((self.raw[self.front + self.nbytes:] == self.PATTERN).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    """bitwise equality of two fp32 tensors (NaN payloads included)"""
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


class Rig:
    """One plan with its device buffers at fixed addresses."""

    def __init__(self, case, precision, B, salt):
        from moleculardiffusion_mivit_amd.engine import MivitPlan
        N = _native()
        cfg = case.cfg
        self.case, self.precision, self.B, self.T = case, precision, B, case.T
        self.scale = LOSS_SCALE[precision]
        self.plan = plan = MivitPlan(
            precision=precision, embedding={"linear": N.EMBED_LINEAR, "cnn": N.EMBED_CNN, "external": N.EMBED_EXTERNAL}[case.embedding],
            patch_size=0 if case.embedding == "external" else cfg.patch_size, embed_dim=cfg.embed_dim, num_heads=cfg.num_heads,
            hidden_dim=cfg.hidden_dim, num_layers=cfg.num_layers,
            activation={"relu": N.ACT_RELU, "leaky_relu": N.ACT_LEAKY_RELU, "gelu": N.ACT_GELU}[cfg.activation],
            use_pos_encoding=cfg.use_pos_encoding, use_regression_token=cfg.use_regression_token,
            fusion={"none": N.FUSION_NONE, "early": N.FUSION_EARLY, "late": N.FUSION_LATE}[case.fusion],
            global_feature_dim=cfg.global_feature_dim or 0, head_hidden=cfg.head_hidden, output_dim=cfg.output_dim)
        assert sorted(plan.param_names) == sorted(param_names(case))
        self.pad = padding_mask(plan).cuda()
        self.arena = pack_arena(plan, orc.closed_form_params(cfg, dtype=torch.float64)).cuda()
        x, labels, feats = batch(case, B, salt, torch.float32)
        self.x, self.labels = x.contiguous().cuda(), labels.cuda()
        self.feats = None if feats is None else feats.contiguous().cuda()
        self.ws = Guarded(plan.workspace_bytes(B, case.T, True), torch.uint8)
        self.out = Guarded(B * cfg.output_dim, torch.float32)
        self.grads = Guarded(plan.arena_numel, torch.float32)
        self.dfeat = Guarded(B * cfg.global_feature_dim, torch.float32) if case.dfeatures else None
        self.dx = Guarded(B * case.T * cfg.embed_dim, torch.float32) if case.dx_tokens else None
        self.dout = torch.zeros(B, cfg.output_dim, device="cuda")
        self.guards = [g for g in (self.ws, self.out, self.grads, self.dfeat, self.dx) if g is not None]

    def _poison(self):
        for g in (self.out, self.grads, self.dfeat, self.dx):
            if g is not None:
                bits(g.t).fill_(SENTINEL)          # the NaN sentinel as a signed word

    def forward(self, ws_fill=None):
        self._poison()
        if ws_fill is not None:
            self.ws.t.fill_(ws_fill)
        self.plan.forward(self.arena, self.x, self.feats, self.B, self.T, self.ws.t, True, self.out.t)
        out = self.out.t.view(self.B, -1)
        self.loss = F.mse_loss(out, self.labels)
        self.dout.copy_((out - self.labels) * (2.0 * self.scale / out.numel()))

    def backward(self, s0=0, s1=None, dfeat=True, dx=True):
        self.plan.backward(self.arena, self.x, self.feats, self.B, self.T, self.ws.t, self.dout, self.grads.t,
                           self.dfeat.t if (self.dfeat is not None and dfeat) else None,
                           self.dx.t if (self.dx is not None and dx) else None, s0, self.plan.num_stages if s1 is None else s1)

    def snapshot(self):
        torch.cuda.synchronize()
        assert all(g.intact() for g in self.guards), "a kernel wrote outside its buffer"
        return SimpleNamespace(out=self.out.t.view(self.B, -1).clone(), loss=self.loss.clone(), arena=self.grads.t.clone(),
                               dfeat=None if self.dfeat is None else self.dfeat.t.clone(),
                               dx=None if self.dx is None else self.dx.t.clone())

    def step(self, ws_fill=None, **kw):
        self.forward(ws_fill)
        self.backward(**kw)
        return self.snapshot()

    def result(self, snap):
        """a snapshot in the oracle's terms: unscaled gradients by reference name"""
        shapes = orc.param_shapes(self.case.cfg)
        cfg = self.case.cfg
        g = {k: (v / self.scale).reshape(shapes[k]) for k, v in unpack_arena(self.plan, snap.arena).items()}
        return SimpleNamespace(out=snap.out, loss=snap.loss, grads=g,
                               dfeatures=None if snap.dfeat is None else (snap.dfeat / self.scale).view(self.B, cfg.global_feature_dim),
                               dx_tokens=None if snap.dx is None else (snap.dx / self.scale).view(self.B, self.T, cfg.embed_dim))


def graph_stats():
    """(replays, captures, failures) of the library's hipGraph cache"""
    import ctypes
    r, c, f = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    _native().lib.mivit_graph_stats(ctypes.byref(r), ctypes.byref(c), ctypes.byref(f))
    return r.value, c.value, f.value
