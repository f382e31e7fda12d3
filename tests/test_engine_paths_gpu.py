"""The engine's dispatch (csrc/engine.hip + the glue kernels of csrc/misc.hip) against the fp64 oracle on every path of the
case table in tests/engine_common.py, in fp32, bf16 and fp16.  MivitPlan.forward / MivitPlan.backward are driven on raw
tensors (the C-ABI with pointer plumbing only): the workspace is exactly workspace_bytes long inside a guarded allocation,
every output is guarded, and the gradient arena starts as NaN, so a wrong offset, a missing zero fill, a wrong leading
dimension or an element nobody writes shows up as an error, a broken guard or a surviving NaN.

fp16 runs its backward under a loss scale of 2**12 (what GradScaler does, as in test_fp16_matches_reference_golden) and the
gradients are unscaled, exactly, before the comparison; bitwise comparisons are made on the scaled values."""
import ctypes
import functools

import pytest
import torch

import engine_common as ec

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ec.CASES]
ALL = [(n, p) for n in NAMES for p in ec.PRECISIONS]
IDS = [f"{n}-{p}" for n, p in ALL]
Guarded, Rig, _bits, _same = ec.Guarded, ec.Rig, ec.bits, ec.same          # (shared with tests/test_graph_replay_gpu.py)


def _native():
    from moleculardiffusion_mivit_amd import _native as N
    return N


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


_graph_stats = ec.graph_stats


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
