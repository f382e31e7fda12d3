"""Readout-row pruning of the last encoder layer (csrc/engine.hip; mivit_set_readout_rows) against the same engine
with the switch off, on the same buffers, driven as tests/test_engine_paths_gpu.py drives it.

The shapes are the smallest that reach each boundary: both fused widths; L = 1 (the last layer is also the first: its q|k|v
backward reads x0 without an input affine) and L = 2; S = 2 (the smallest sequence with a pruned row), 33 (three 16-row
tiles, the benchmark's) and 64 (the largest fused sequence); B = 1 (one partial 32-row tile of the compact launches), 24 and 33
(one row over a tile); bf16 and fp16; one early-fusion case (the regression row is reg + fp_out).

The switch has three values: 0 = every row, 1 (default) = the pruning that leaves every sum as it was (the feed-forward
block's forward and the attention core's backward), 2 = also the feed-forward and LayerNorm-1 / out-projection backward on B rows.

What must hold:
 * out and loss: bitwise equal between the modes (a row's forward result does not depend on where in a tile it sits);
 * mode 1: EVERY gradient equal to mode 0 as values (torch.equal: only the sign of a zero may differ);
 * mode 2: every gradient outside the last layer's fc1 / fc2 / norm2 / out_proj / norm1 equal as values;
 * those ten tensors hold, in mode 2, the same fp32 terms summed in another order: per tensor ||diff|| <= 1e-5 (||g|| + 1e-2 x the largest
   gradient norm), the measure of engine_common.lowp_errors; reorder noise at these row counts is 2^-24 sqrt(rows) < 1e-6;
 * in all three modes: the accuracy bound of test_accuracy_against_fp64, intact guards, no NaN in the arena after a workspace of
   0xFF bytes, staged backward bitwise equal to the single call;
 * toggling the switch between calls with identical arguments gives the result of the mode in force, not a replayed graph."""
import functools

import pytest
import torch

import engine_common as ec
from oracle import mivit_oracle as orc
from test_engine_paths_gpu import Rig, _bits, _native, _same

pytestmark = pytest.mark.gpu

REORDER_TOL = 1e-5
LOWP_KINK = 2.0 ** -8          # one bf16 rounding step at 1
WIDTHS = ((128, 256, 4), (64, 128, 4))
CASES = [ec.Case(f"rr_w{E}_L{L}_S{S}", ec._cfg(E, H, Fh, L), S - 1, "linear", "fused")
         for E, Fh, H in WIDTHS for L in (1, 2) for S in (2, 33, 64)]
EARLY = ec.Case("rr_w128_early_S14", ec._cfg(128, 4, 256, 1, "leaky_relu", use_global_features=True, fusion_type="early",
                                             global_feature_dim=25), 13, "linear", "fused", dfeatures=True)
for _c in CASES + [EARLY]:
    ec.CASE_BY_NAME.setdefault(_c.name, _c)          # (the oracles of engine_common look a case up by name)
PARAMS = [(c.name, B, p) for c in CASES for B in (1, 24, 33) for p in ("bf16", "fp16")] + [(EARLY.name, 24, p) for p in ("bf16", "fp16")]
IDS = [f"{n}-B{B}-{p}" for n, B, p in PARAMS]
MODES = {"exact": 1, "all": 2, "off": 0}


def _pruned_names(case):
    pre = f"transformer.encoder_layers.{case.cfg.num_layers - 1}."
    return {pre + blk + "." + wb for blk in ("feed_forward.fc1", "feed_forward.fc2", "norm2", "self_attn.out_proj", "norm1")
            for wb in ("weight", "bias")}


@functools.lru_cache(maxsize=None)
def _salt(name, B):
    """The input salt of a case.  engine_common.pick_salt keeps every ReLU pre-activation clear of fp32 noise; where even that
    fails among its 64 salts (33 x 64 rows hold a million pre-activations) the 16-bit runs here take salt 0: their own rounding
    is a thousand times coarser than that margin anyway, and over >= 24 sequences a flipped ReLU averages out (Case.batches).
    A single sequence has nothing to average over: B = 1 takes the first salt whose pre-activations clear a bf16 rounding step,
    if there is one (there is at S = 2)."""
    case = ec.CASE_BY_NAME[name]
    if B == 1:
        p = orc.closed_form_params(case.cfg, dtype=torch.float64)
        for salt in range(64):
            frames, _, _, feats = ec._batch64(name, 1, salt)
            if orc.min_kink_margin(p, case.cfg, frames, feats) > LOWP_KINK:
                return salt
    salt = ec.pick_salt(case, B)
    return 0 if salt is None else salt


class _Switch:
    def __init__(self, mode):
        self.value = MODES[mode]

    def __enter__(self):
        self.old = _native().lib.mivit_set_readout_rows(self.value)

    def __exit__(self, *exc):
        _native().lib.mivit_set_readout_rows(self.old)


def _staged(rig):
    """forward, then one backward call per stage -> (snapshot, [copy of each stage's range right after its call])"""
    rig.forward(0x00)
    copies = []
    for s, (b, e) in enumerate(rig.plan.stage_ranges):
        rig.backward(s, s + 1)
        copies.append(rig.grads.t[b:e].clone())
    return rig.snapshot(), copies


@functools.lru_cache(maxsize=None)
def _runs(name, B, precision):
    """One rig; per mode: a step on a workspace of 0x00 bytes, one on 0xFF bytes, a staged backward -- all on the same buffers"""
    case = ec.CASE_BY_NAME[name]
    salt = _salt(name, B)
    rig = Rig(case, precision, B, salt)
    rig.salt = salt
    runs = {}
    for mode in MODES:
        with _Switch(mode):
            zero, ones = rig.step(0x00), rig.step(0xFF)
            staged, copies = _staged(rig)
        runs[mode] = (zero, ones, staged, copies)
    return rig, runs


@pytest.mark.parametrize("name,B,precision", PARAMS, ids=IDS)
def test_modes_agree(name, B, precision):
    rig, runs = _runs(name, B, precision)
    on, off, exact = runs["all"][0], runs["off"][0], runs["exact"][0]
    for snap in (on, exact):
        assert _same(snap.out, off.out) and _same(snap.loss.reshape(1), off.loss.reshape(1)), "a row's forward result depends on the mode"
    g_on, g_off = ec.unpack_arena(rig.plan, on.arena), ec.unpack_arena(rig.plan, off.arena)
    unequal = [k for k, v in ec.unpack_arena(rig.plan, exact.arena).items() if not torch.equal(v, g_off[k])]
    assert not unequal, ("mode 1 changed a gradient", unequal)
    assert exact.dfeat is None or torch.equal(exact.dfeat, off.dfeat)
    pruned = _pruned_names(rig.case)
    assert pruned <= set(g_on)
    unequal = [k for k in g_on if k not in pruned and not torch.equal(g_on[k], g_off[k])]
    assert not unequal, unequal
    assert on.dfeat is None or torch.equal(on.dfeat, off.dfeat)
    gscale = max(float(v.double().norm()) for v in g_off.values())
    err = {k: float((g_on[k].double() - g_off[k].double()).norm()) / (float(g_off[k].double().norm()) + 1e-2 * gscale) for k in pruned}
    worst = max(err, key=err.get)
    print(f"READOUT-ROWS {name} B={B} {precision}: worst reorder difference {err[worst]:.2e} ({worst})")
    assert err[worst] <= REORDER_TOL, (worst, err[worst])


@pytest.mark.parametrize("name,B,precision", PARAMS, ids=IDS)
def test_every_mode_holds_the_engine_contract(name, B, precision):
    """(guards: every snapshot of _runs asserts them)"""
    rig, runs = _runs(name, B, precision)
    ref, yard = ec.reference(rig.case, B, rig.salt), None
    for mode in MODES:
        zero, ones, staged, copies = runs[mode]
        # the 0xFF workspace: nothing unwritten is read
        assert bool(torch.isfinite(ones.arena[~rig.pad]).all()), mode
        assert _same(zero.out, ones.out) and _same(zero.arena, ones.arena), mode
        assert zero.dfeat is None or _same(zero.dfeat, ones.dfeat), mode
        # staged backward: final per stage, bitwise the single call
        for s, (b, e) in enumerate(rig.plan.stage_ranges):
            assert _same(copies[s], staged.arena[b:e]), (mode, f"stage {s}'s range was written by a later stage")
            assert _same(copies[s], zero.arena[b:e]), (mode, f"stage {s} differs from the single-call backward")
        assert _same(staged.out, zero.out) and (zero.dfeat is None or _same(staged.dfeat, zero.dfeat)), mode
        # accuracy: the bound of test_accuracy_against_fp64
        got = rig.result(zero)
        assert bool(torch.isfinite(got.out).all())
        err = ec.lowp_errors(got, ref)
        yard = yard or ec.lowp_errors(ec.yardstick(rig.case, B, rig.salt), ref)
        gk = [k for k in err if k not in ("out", "loss")]
        wk = max(gk, key=err.get)
        print(f"READOUT-ROWS {name} B={B} {precision} {mode}: out {err['out']:.1e} (yardstick {yard['out']:.1e}) loss {err['loss']:.1e} "
              f"({yard['loss']:.1e}) worst grad {err[wk]:.1e} ({yard[wk]:.1e}) {wk}")
        for k in err:
            assert err[k] <= 3 * yard[k] + ec.lowp_floor(k), (mode, k, err[k], yard[k])


@pytest.mark.parametrize("precision", ("bf16", "fp16"))
def test_toggling_the_switch_is_not_a_stale_replay(precision):
    """A graph-sized shape, identical arguments throughout: three calls per mode (direct, captured, replayed), then the modes
    alternate.  Every call gives what its mode gave the first time, and modes 2 and 0 do differ at this shape (otherwise this
    test could not tell them apart; mode 1 equals mode 0 by design)."""
    name = "rr_w128_L2_S33"
    case = ec.CASE_BY_NAME[name]
    rig = Rig(case, precision, 24, _salt(name, 24))
    first = {}
    for mode in MODES:
        with _Switch(mode):
            snaps = [rig.step(0x00) for _ in range(3)]
        first[mode] = snaps[0]
        assert all(_same(s.arena, snaps[0].arena) and _same(s.out, snaps[0].out) for s in snaps[1:]), mode
    assert not _same(first["all"].arena, first["off"].arena), "modes 2 and 0 are bitwise equal here: pick another shape"
    for mode in ("all", "off", "exact", "all", "off"):
        with _Switch(mode):
            snap = rig.step(0x00)
        assert _same(snap.out, first[mode].out) and _same(snap.arena, first[mode].arena), f"mode {mode} replayed the other mode's graph"


def test_switch_returns_the_previous_value():
    lib = _native().lib
    old = lib.mivit_set_readout_rows(0)
    assert lib.mivit_set_readout_rows(1) == 0 and lib.mivit_set_readout_rows(old) == 1
