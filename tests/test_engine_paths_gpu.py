"""The engine's dispatch (csrc/engine.hip + the glue kernels of csrc/misc.hip) against the fp64 oracle on every path of the
case table in tests/engine_common.py, in fp32, bf16 and fp16.  MivitPlan.forward / MivitPlan.backward are driven on raw
tensors (the C-ABI with pointer plumbing only): the workspace is exactly workspace_bytes long inside a guarded allocation,
every output is guarded, and the gradient arena starts as NaN, so a wrong offset, a missing zero fill, a wrong leading
dimension or an element nobody writes shows up as an error, a broken guard or a surviving NaN.

fp16 runs its backward under a loss scale of 2**12 (what GradScaler does, as in test_fp16_matches_reference_golden) and the
gradients are unscaled, exactly, before the comparison; bitwise comparisons are made on the scaled values."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import engine_common as ec
from oracle import mivit_oracle as orc

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ec.CASES]
ALL = [(n, p) for n in NAMES for p in ec.PRECISIONS]
IDS = [f"{n}-{p}" for n, p in ALL]
LOSS_SCALE = {"fp32": 1.0, "bf16": 1.0, "fp16": 4096.0}
GUARD_BYTES = 4096


def _native():
    from moleculardiffusion_mivit_amd import _native as N
    return N


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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """bitwise equality of two fp32 tensors (NaN payloads included)"""
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


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
        assert sorted(plan.param_names) == sorted(ec.param_names(case))
        self.pad = ec.padding_mask(plan).cuda()
        self.arena = ec.pack_arena(plan, orc.closed_form_params(cfg, dtype=torch.float64)).cuda()
        x, labels, feats = ec.batch(case, B, salt, torch.float32)
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
                _bits(g.t).fill_(ec.SENTINEL)          # the NaN sentinel as a signed word

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
        g = {k: (v / self.scale).reshape(shapes[k]) for k, v in ec.unpack_arena(self.plan, snap.arena).items()}
        return SimpleNamespace(out=snap.out, loss=snap.loss, grads=g,
                               dfeatures=None if snap.dfeat is None else (snap.dfeat / self.scale).view(self.B, cfg.global_feature_dim),
                               dx_tokens=None if snap.dx is None else (snap.dx / self.scale).view(self.B, self.T, cfg.embed_dim))


@functools.lru_cache(maxsize=None)
def _rig(name, precision, B):
    """One rig per (case, precision, batch) for the whole module, with the two runs every test starts from: `zero` on a
    workspace of 0x00 bytes, `ones` the same call sequence on the same buffers after filling the workspace with 0xFF bytes
    (NaN in all three element types)."""
    case = ec.CASE_BY_NAME[name]
    salt = ec.pick_salt(case, B)
    assert salt is not None
    rig = Rig(case, precision, B, salt)
    rig.salt = salt
    rig.zero = rig.step(0x00)
    rig.ones = rig.step(0xFF)
    return rig


def _rigs(name, precision):
    return [_rig(name, precision, B) for B in ec.CASE_BY_NAME[name].batches(precision)]


def _graph_stats():
    r, c, f = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    _native().lib.mivit_graph_stats(ctypes.byref(r), ctypes.byref(c), ctypes.byref(f))
    return r.value, c.value, f.value


# ---- a. accuracy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ALL, ids=IDS)
def test_accuracy_against_fp64(name, precision):
    """fp32: out, loss, every parameter gradient, d(features) and d(tokens) within FP32_TOL of the fp64 oracle (gradients per
    tensor, scaled as _grad_err of test_model_gpu.py).  bf16 and fp16: error against fp64 at most 3 x the error of PyTorch's own
    bf16 autocast of the oracle on the same inputs, plus the floors of test_bf16_as_accurate_as_torch_autocast (fp16 rounds 8 x
    finer than bf16, so the bf16 yardstick is an upper bound for it by construction).  Measured figures: DESIGN.md."""
    for rig in _rigs(name, precision):
        ref = ec.reference(rig.case, rig.B, rig.salt)
        got = rig.result(rig.zero)
        assert bool(torch.isfinite(got.out).all())
        if precision == "fp32":
            err = ec.fp32_errors(got, ref)
            worst = max(err, key=err.get)
            print(f"ENGINE-PATHS {name} {precision} B={rig.B}: out {err['out']:.1e} loss {err['loss']:.1e} worst grad "
                  f"{max((v, k) for k, v in err.items() if k not in ('out', 'loss'))}")
            assert err[worst] < ec.FP32_TOL, (rig.B, worst, err[worst])
        else:
            err, yard = ec.lowp_errors(got, ref), ec.lowp_errors(ec.yardstick(rig.case, rig.B, rig.salt), ref)
            gk = [k for k in err if k not in ("out", "loss")]
            wk = max(gk, key=err.get)
            print(f"ENGINE-PATHS {name} {precision} B={rig.B}: out {err['out']:.1e} (yardstick {yard['out']:.1e}) loss "
                  f"{err['loss']:.1e} ({yard['loss']:.1e}) worst grad {err[wk]:.1e} ({yard[wk]:.1e}) {wk}")
            for k in err:
                assert err[k] <= 3 * yard[k] + ec.lowp_floor(k), (k, err[k], yard[k])


# ---- b. path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ALL, ids=IDS)
def test_case_runs_on_the_expected_path(name, precision):
    """One more forward + backward with the in-library profiler on (it brackets the main kernel of every tagged launch): the
    fused cases launch the fused blocks once per layer and the general attention never; the per-operator cases and every fp32
    case the reverse.  A case that silently falls to the other path fails here instead of passing on the wrong kernel."""
    N = _native()
    rig = _rigs(name, precision)[0]
    L = rig.case.cfg.num_layers
    counts = {}
    try:
        N.check(N.lib.mivit_profile_enable((1 << len(N.PROF_TAGS)) - 1), "profile_enable")
        snap = rig.step()
    finally:
        N.lib.mivit_profile_enable(0)
        for i, tag in enumerate(N.PROF_TAGS):
            ms, n = ctypes.c_double(), ctypes.c_int()
            N.lib.mivit_profile_collect(i, ctypes.byref(ms), ctypes.byref(n))
            counts[tag] = n.value
    fused = rig.case.path == "fused" and precision != "fp32"
    if fused:
        assert (counts["attn_block_fwd"], counts["mlp_block_fwd"], counts["mlp_block_bwd"], counts["attn_out_bwd"]) == (L, L, L, L), counts
        assert counts["attn_fwd"] == 0 and counts["attn_bwd"] == 0 and counts["attn_core_bwd"] == L, counts
    else:
        assert counts["attn_fwd"] == L and counts["attn_bwd"] == L, counts
        assert all(counts[t] == 0 for t in ("attn_block_fwd", "mlp_block_fwd", "mlp_block_bwd", "attn_out_bwd", "attn_core_bwd",
                                            "qkv_bwd")), counts
    # the profiler only brackets launches: the results are those of the plain run
    assert _same(snap.out, rig.zero.out) and _same(snap.arena, rig.zero.arena)


# ---- c. bounds and overwrite --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ALL, ids=IDS)
def test_every_parameter_gradient_is_overwritten_and_nothing_else(name, precision):
    """Into an arena of NaN: every parameter element comes back finite (the rows of the positional table beyond the sequence
    exactly 0), the padding between tensors keeps its NaN word, and every guard is intact (checked by each snapshot)."""
    for rig in _rigs(name, precision):
        for snap in (rig.zero, rig.ones):
            left = {k: int(torch.isnan(v).sum()) for k, v in ec.unpack_arena(rig.plan, snap.arena).items() if bool(torch.isnan(v).any())}
            assert not left, f"parameter gradient elements never written: {left}"
            assert bool(torch.isfinite(snap.arena[~rig.pad]).all())
            assert bool((_bits(snap.arena)[rig.pad] == ec.SENTINEL).all()), "arena padding was written"
            if rig.case.cfg.use_pos_encoding:
                E, S = rig.case.cfg.embed_dim, rig.case.S
                pos = ec.unpack_arena(rig.plan, snap.arena)["transformer.pos_embedding"].view(128, E)
                assert bool((_bits(pos[S:]) == 0).all()) and bool((pos[:S] != 0).any())
            for t in (snap.dfeat, snap.dx):
                assert t is None or bool(torch.isfinite(t).all())


# ---- d. workspace independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ALL, ids=IDS)
def test_results_do_not_depend_on_what_the_workspace_held(name, precision):
    for rig in _rigs(name, precision):
        a, b = rig.zero, rig.ones
        assert _same(a.out, b.out)
        diff = [k for k, v in ec.unpack_arena(rig.plan, a.arena).items() if not _same(v, ec.unpack_arena(rig.plan, b.arena)[k])]
        assert not diff, diff
        assert _same(a.arena, b.arena)
        assert (a.dfeat is None or _same(a.dfeat, b.dfeat)) and (a.dx is None or _same(a.dx, b.dx))


# ---- e. staged backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ALL, ids=IDS)
def test_staged_backward_finalises_each_stage_range(name, precision):
    """What dp.py relies on when it all-reduces stage_range(s) as soon as stage s is queued: after backward(s, s + 1) the range
    is final -- no later stage writes it -- and it is bitwise what the single-call backward produces."""
    for rig in _rigs(name, precision):
        plan = rig.plan
        assert plan.num_stages == rig.case.cfg.num_layers + 2
        assert plan.stage_ranges[0][0] == 0 and plan.stage_ranges[-1][1] == plan.arena_numel
        assert all(plan.stage_ranges[s][1] == plan.stage_ranges[s + 1][0] for s in range(plan.num_stages - 1))
        rig.forward(0x00)
        copies = []
        for s in range(plan.num_stages):
            rig.backward(s, s + 1)
            b, e = plan.stage_ranges[s]
            copies.append(rig.grads.t[b:e].clone())
            if s + 1 < plan.num_stages:          # nothing of the stages still to come has been written
                assert bool((_bits(rig.grads.t[e:]) == ec.SENTINEL).all()), s
        end = rig.snapshot()
        for s, (b, e) in enumerate(plan.stage_ranges):
            assert _same(copies[s], end.arena[b:e]), f"stage {s}'s range was written by a later stage"
            assert _same(copies[s], rig.zero.arena[b:e]), f"stage {s} differs from the single-call backward"
        assert _same(end.out, rig.zero.out)
        assert (end.dfeat is None or _same(end.dfeat, rig.zero.dfeat)) and (end.dx is None or _same(end.dx, rig.zero.dx))


# ---- f. optional outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [(n, p) for n, p in ALL if ec.CASE_BY_NAME[n].dfeatures or ec.CASE_BY_NAME[n].dx_tokens],
                         ids=[i for i, (n, p) in zip(IDS, ALL) if ec.CASE_BY_NAME[n].dfeatures or ec.CASE_BY_NAME[n].dx_tokens])
def test_optional_outputs_do_not_change_the_parameter_gradients(name, precision):
    for rig in _rigs(name, precision):
        combos = {(False, False)}
        if rig.dfeat is not None and rig.dx is not None:
            combos |= {(True, False), (False, True)}
        for want_f, want_x in sorted(combos):
            snap = rig.step(0x00, dfeat=want_f, dx=want_x)
            assert _same(snap.arena, rig.zero.arena), (want_f, want_x)
            for g, want, ref in ((snap.dfeat, want_f, rig.zero.dfeat), (snap.dx, want_x, rig.zero.dx)):
                if g is None:
                    continue
                if want:
                    assert _same(g, ref)
                else:                              # not requested: not touched
                    assert bool((_bits(g) == ec.SENTINEL).all())


# ---- g. direct call, capture, replay ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.GRAPH_CASES)
@pytest.mark.parametrize("precision", ec.PRECISIONS)
def test_direct_captured_and_replayed_calls_agree_bitwise(name, precision):
    """Same addresses three times: call 1 runs the kernels directly, call 2 captures them into a hipGraph, call 3 replays it
    (a fresh plan, so no key has been seen before)."""
    case = ec.CASE_BY_NAME[name]
    B = case.batches(precision)[0]
    rig = Rig(case, precision, B, ec.pick_salt(case, B))
    r0, c0, f0 = _graph_stats()
    runs = [rig.step(0x00 if i != 1 else 0xFF) for i in range(3)]
    r1, c1, f1 = _graph_stats()
    assert f1 == f0, "hipGraph capture failed"
    assert (c1 - c0, r1 - r0) == (2, 2), (c1 - c0, r1 - r0)          # forward + backward: captured once, replayed once
    for snap in runs[1:]:
        assert _same(snap.out, runs[0].out) and _same(snap.arena, runs[0].arena)
        assert (snap.dfeat is None or _same(snap.dfeat, runs[0].dfeat)) and (snap.dx is None or _same(snap.dx, runs[0].dx))
    shared = _rig(name, precision, B)
    assert _same(runs[0].out, shared.zero.out) and _same(runs[0].arena, shared.zero.arena)          # another plan, other addresses
