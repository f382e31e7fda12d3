"""Host side of the engine-dispatch suite: the case table of tests/engine_common.py covers the branches it claims, every case
has a well-conditioned input, and the references the device test relies on are sound on their own (the fp32 oracle sits far
inside the fp32 gate, the bf16 yardstick is finite and alive, the trunk-from-tokens oracle is the oracle)."""
import math

import pytest
import torch

import engine_common as ec
from oracle import mivit_oracle as orc

NAMES = [c.name for c in ec.CASES]


def _salted(case, precision):
    return [(B, ec.pick_salt(case, B)) for B in case.batches(precision)]


@pytest.mark.parametrize("name", NAMES)
def test_every_case_has_a_salt_clear_of_the_relu_kinks(name):
    case = ec.CASE_BY_NAME[name]
    for prec in ("fp32", "bf16"):
        for B, salt in _salted(case, prec):
            assert salt is not None, (name, B)
            frames, _, _, feats = ec._batch64(name, B, salt)
            p = orc.closed_form_params(case.cfg, dtype=torch.float64)
            assert orc.min_kink_margin(p, case.cfg, frames, feats) > ec.KINK_MARGIN


@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_is_well_inside_the_fp32_gate(name):
    """fp32 arithmetic itself (the oracle in fp32 on the rounded inputs) against the fp64 reference: a tenth of FP32_TOL on out,
    loss and every gradient, in the device test's own measure.  A case that misses is badly conditioned, not a kernel bug."""
    case = ec.CASE_BY_NAME[name]
    for B, salt in _salted(case, "fp32"):
        err = ec.fp32_errors(ec.oracle_fp32(case, B, salt), ec.reference(case, B, salt))
        worst = max(err, key=err.get)
        print(f"{name} B={B} salt={salt}: fp32 oracle vs fp64 worst {worst} {err[worst]:.2e}")
        assert err[worst] < 0.1 * ec.FP32_TOL, (B, worst, err[worst])
        assert set(err) == {"out", "loss"} | set(ec.param_names(case)) | ({"d(features)"} if case.dfeatures else set()) \
            | ({"d(tokens)"} if case.dx_tokens else set())


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_is_finite_and_not_degenerate(name):
    case = ec.CASE_BY_NAME[name]
    (B, salt), = _salted(case, "bf16")
    ref, y = ec.reference(case, B, salt), ec.yardstick(case, B, salt)
    assert y.out.dtype == torch.float32 and y.out.shape == (B, case.cfg.output_dim)
    for k, (t, _) in ec._tensors(y).items():
        assert bool(torch.isfinite(t).all()), k
    err = ec.lowp_errors(y, ref)
    print(f"{name}: yardstick out {err['out']:.2e} loss {err['loss']:.2e} worst grad "
          f"{max(v for k, v in err.items() if k not in ('out', 'loss')):.2e}")
    # alive: bf16 rounding is visible (an "autocast" that silently ran fp32 would sit at 1e-7) but the result is the same model
    assert 1e-5 < err["out"] < 0.2 and all(math.isfinite(v) and v < 0.5 for v in err.values()), err
    assert float(ref.out.std()) > 1e-3 and float(ref.loss) > 1e-4          # outputs differ between sequences, loss is not 0
    for k, g in ref.grads.items():
        if "k_proj.bias" in k or (case.S == 1 and ("q_proj" in k or "k_proj" in k)):
            continue      # analytically zero: softmax is shift-invariant / a single token attends to itself
        if case.cfg.num_layers == 0 and case.cfg.use_regression_token and k.startswith(("embedding.", "norm.")):
            continue      # without a layer the regression-token readout never sees the frames
        assert float(g.abs().max()) > 0, k


@pytest.mark.parametrize("name", NAMES)
def test_trunk_from_tokens_is_the_forward_bitwise(name):
    case = ec.CASE_BY_NAME[name]
    cfg = case.cfg
    for dtype in (torch.float32, torch.float64):
        p = orc.closed_form_params(cfg, dtype=dtype)
        frames, _, _, feats = (None if t is None else t.to(dtype) for t in ec._batch64(name, 3, 0))
        a, b = {}, {}
        out = orc.forward(p, cfg, frames, feats, trace=a)
        out2 = orc.forward_from_tokens(p, cfg, orc.embed(p, cfg, frames), feats, trace=b)
        assert torch.equal(out, out2)
        assert torch.equal(a["x0"], b["x0"]) and torch.equal(a["pooled"], b["pooled"])


def test_external_reference_differentiates_the_tokens():
    """d(tokens) of the trunk-from-tokens reference is the gradient the frames' embedding would have received: pushed through
    the linear embedding by hand it gives the embedding gradients of the whole-model oracle."""
    case = ec.CASE_BY_NAME["external_w64"]
    ref = ec.reference(case, 3, 0)
    frames, _, labels, _ = ec._batch64(case.name, 3, 0)
    p = orc.closed_form_params(case.cfg, dtype=torch.float64)
    _, _, g = orc.loss_and_grads(p, case.cfg, frames, labels)
    dW = ref.dx_tokens.reshape(-1, 64).T @ frames.reshape(-1, 81)
    assert torch.allclose(dW, g["embedding.proj.weight"], rtol=1e-10, atol=1e-14)
    assert torch.allclose(ref.dx_tokens.sum(dim=(0, 1)), g["embedding.proj.bias"], rtol=1e-10, atol=1e-14)
    assert "embedding.proj.weight" not in ref.grads and ref.dx_tokens.shape == (3, 11, 64)


def test_table_covers_every_branch():
    C = ec.CASES
    assert len({c.name for c in C}) == len(C) == 19
    assert {c.cfg.activation for c in C if c.cfg.num_layers} == {"relu", "leaky_relu", "gelu"}
    assert {c.fusion for c in C} == {"none", "early", "late"}
    assert {c.cfg.use_regression_token for c in C} == {True, False}
    assert {c.cfg.use_pos_encoding for c in C} == {True, False}
    assert {c.embedding for c in C} == {"linear", "cnn", "external"}
    assert any(c.cfg.num_layers == 0 for c in C)
    assert {1, 2, 64, 65} <= {c.S for c in C}
    assert {c.path for c in C} == {"fused", "per_operator", "none"}
    assert all((c.path == "none") == (c.cfg.num_layers == 0) for c in C)
    # the expected path restates fused_layer_supported (csrc/fused_fwd.hip): the two compiled widths, at most 64 tokens
    for c in C:
        g = c.cfg
        fusable = (g.embed_dim, g.hidden_dim, g.num_heads) in ((64, 128, 4), (128, 256, 4)) and c.S <= 64
        assert c.path == ("none" if g.num_layers == 0 else "fused" if fusable else "per_operator"), c.name
    # both sides of the switch at both fused widths, and the neighbours that differ in one number only
    for E in (64, 128):
        assert {c.path for c in C if c.cfg.embed_dim == E and c.cfg.hidden_dim == 2 * E and c.cfg.num_heads == 4
                and c.cfg.num_layers} == {"fused", "per_operator"}
    # stage-0 readout variants: mean-pool + late fusion (the strided convert), output_dim > 1, a head width off the 8-grid
    assert any(not c.cfg.use_regression_token and c.fusion == "late" and c.dfeatures for c in C)
    assert any(c.cfg.output_dim > 1 and c.cfg.head_hidden % 8 for c in C)
    assert any(c.cfg.global_feature_dim and c.cfg.global_feature_dim % 8 for c in C)
    assert any(c.dx_tokens for c in C) and all(c.dx_tokens == (c.embedding == "external") for c in C)
    assert all(not c.dfeatures or c.fusion != "none" for c in C)
    assert any(c.fp32_B1 for c in C)
    assert all(c.cfg.patch_size == 9 for c in C)
    assert {24 * c.T >= 256 for c in C if c.embedding != "external"} == {True, False}      # small-frame embedding kernels on / off
    assert set(ec.GRAPH_CASES) <= set(ec.CASE_BY_NAME)
    assert all(c.embedding == "external" or c.cfg.embedding == c.embedding for c in C)


def test_pack_arena_places_parameters_and_pads_with_the_sentinel():
    from types import SimpleNamespace
    plan = SimpleNamespace(param_names=["b", "a"], param_offsets=[0, 8], param_numels=[3, 5], arena_numel=16)
    params = {"a": torch.arange(5.0).reshape(1, 5), "b": -torch.ones(3, dtype=torch.float64)}
    arena = ec.pack_arena(plan, params)
    assert arena.dtype == torch.float32 and arena.numel() == 16
    assert torch.equal(arena[0:3], -torch.ones(3)) and torch.equal(arena[8:13], torch.arange(5.0))
    pad = ec.padding_mask(plan)
    assert pad.tolist() == [False] * 3 + [True] * 5 + [False] * 5 + [True] * 3
    assert bool((arena.view(torch.int32)[pad] == ec.SENTINEL).all()) and bool(torch.isnan(arena[pad]).all())
    got = ec.unpack_arena(plan, arena)
    assert torch.equal(got["a"], torch.arange(5.0))
