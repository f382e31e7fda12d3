"""The hipGraph cache (graph_run, csrc/misc.hip) between the caller and every kernel of mivit_forward / mivit_backward /
mivit_deepresnet_train_fwd / _bwd on launch-bound problems: the first call with an argument tuple runs the kernels directly,
the second captures them on an internal stream, every later one replays the graph on the caller's stream.  The kernels are
not under test here (tests/test_engine_paths_gpu.py and the DeepResNet Walk hold them to fp64); the layer that decides
between running and replaying is.

Authority: the same contents run through a FRESH rig -- a new plan has a uid no key has seen, so its calls are first
sightings and run directly, which every fresh run asserts with mivit_graph_stats (neither `captures` nor `replays` moves).
Every comparison is bitwise.  Every step poisons its outputs first (a replay that writes nothing leaves the sentinel behind),
checks the guards and that `failures` did not move, and asserts the counters PER LIBRARY CALL: direct (0 captures, 0
replays), capture (1, 0), replay (0, 1).  Step A2 of section 1 additionally runs the fp64 comparison of
test_accuracy_against_fp64 on the replayed result, bars unchanged.

  1. contents change at fixed addresses (engine)      test_contents_change_at_fixed_addresses
  2. one pointer of the key changes                    test_a_changed_pointer_is_a_new_key, test_need_backward_is_in_the_key,
                                                       test_stage_range_is_in_the_key
  3. capture on one stream, replay on others           test_replay_on_other_streams_is_ordered_on_the_callers_stream
  4. LRU eviction                                      test_evicted_key_starts_over
  5. DeepResNet training entries                       test_deepresnet_replays_read_live_state, test_deepresnet_momentum_eps_in_key
  6. run-time switches, MIVIT_GRAPHS=0                 test_switch_change_starts_the_key_over, test_graphs_disabled_by_environment
  7. a training loop at model level                    test_training_loop_equals_the_unreplayed_loop

Run-time switches (section 6).  Every setter below bumps the switch epoch that graph_run appends to every key (misc.hip:
graph_switch_changed), in every element-type build; the fused blocks' 64-wide build has no setter (its wave count is fixed).
SWITCHES lists, per setter, where the engine reads the value and the case that reaches it.  mivit_set_readout_rows stays in
the two hand-written engine keys (tests/test_readout_rows_gpu.py, tests/test_readout_query_gpu.py).  No setter reaches a
DeepResNet call: csrc/deepresnet_train.hip launches only its own kernels and launch_slab_reduce, which reads no switch.

MUTATION RECORD (scratch copies of the library, never committed).
Mutations, each a run of its own of the whole module (126 tests); none faulted:
  (a) `(uint64_t)dout` dropped from the backward key (engine.hip): 9 fail, test_a_changed_pointer_is_a_new_key[*-dout] in all
      9 case x precision combinations: "second dout buffer, sighting as direct backward: expected a direct call (captures,
      replays) += (0, 0), counters moved by (0, 1)".
  (b) `(uint64_t)out` dropped from the forward key: 10 fail, test_a_changed_pointer_is_a_new_key[*-out] x 9: "second out
      buffer, sighting as direct forward: expected a direct call ... counters moved by (0, 1)", and
      test_evicted_key_starts_over: "key 1 as direct: expected a direct call ... counters moved by (1, 0)".
  (c) the replay branch returns 0 without hipGraphLaunch (misc.hip): 122 fail, every test that replays, at its first replay:
      "first buffer replay: out still holds the sentinel in every word: the call wrote nothing into this buffer; arena still
      holds the sentinel ..." (test_contents_change_at_fixed_addresses at "A2 Contents(x=1, feats=1, labels=0,
      params='closed')", the stream test at "replay on a stream of its own").
  (d) the LRU evicts the MOST recently used entry: 119 fail as soon as the table is full, because the key just remembered is
      the one evicted: "A1 ... forward: expected a capture call (captures, replays) += (1, 0), counters moved by (0, 0)" in
      every engine test, "F1: expected a capture call ..." in test_deepresnet_replays_read_live_state,
      test_evicted_key_starts_over likewise, and test_training_loop_equals_the_unreplayed_loop: "the loop with graphs never
      replayed: ...".
  (e) the switch epoch left out of the key (misc.hip), which is the parent commit's behaviour: 11 fail, every case of
      test_switch_change_starts_the_key_over: "after mivit_rowstream_set_wavestream(0) (was 2) forward: expected a direct
      call (captures, replays) += (0, 0), counters moved by (0, 1)", and the same for mivit_mlp_block_bwd_set_waves(4) (was
      8), mivit_rowstream_set_wavestream_mask(0) (was 7), mivit_wgrad_bf16_set_config(21) (was 0),
      mivit_embed_set_variant(3) (was 0), mivit_gemm_dma_set_variant(9) (was 0).
  (f) `momentum` dropped from the DeepResNet forward key (deepresnet_train.hip): 2 fail,
      test_deepresnet_momentum_eps_in_key[momentum-f32 / -bf16]: "momentum changed: expected a direct call ... counters
      moved by (0, 1)".
  MIVIT_GRAPHS=0 needed no library change: test_graphs_disabled_by_environment passes on the parent's graph_run as well.
Run time on the MI355X: all 126 tests 14.1 s including start-up; the slowest are test_graphs_disabled_by_environment (2.6 s,
a child process), test_training_loop_equals_the_unreplayed_loop[linear-bf16] (1.8 s) and the first switch test of the
per-operator case (1.8 s, it builds that case's references); every other test is below 1 s.
"""
import ctypes
import functools
import math
import os
import subprocess
import sys
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import deepresnet_common as dc
import engine_common as ec
from oracle import mivit_oracle as orc

pytestmark = pytest.mark.gpu

same, bits, stats = ec.same, ec.bits, ec.graph_stats
CASES = ("w64_fused_S12", "w128_meanpool_late_out3", "external_w32_gelu_meanpool_late")
GRID = [(n, p) for n in CASES for p in ec.PRECISIONS]
GRID_IDS = [f"{n}-{p}" for n, p in GRID]
DELTA = {"direct": (0, 0), "capture": (1, 0), "replay": (0, 1)}          # (captures, replays) of ONE library call

# Shapes that reach the two switches no case of the engine table reaches (a 16 x 16 patch for the LDS-DMA embedding, a
# feed-forward width beyond the row-stream kernels for the wide-layer GEMMs); known to this module only.
_EXTRA = [
    ec.Case("w128_P16_embed_dma", orc.MiViTConfig(embedding="linear", patch_size=16, embed_dim=128, num_heads=4, hidden_dim=256,
                                                  num_layers=1, activation="relu"), 11, "linear", "fused"),
    ec.Case("w128_hidden512", orc.MiViTConfig(embedding="linear", patch_size=ec.PATCH, embed_dim=128, num_heads=4, hidden_dim=512,
                                              num_layers=1, activation="relu"), 11, "linear", "per_operator"),
]
for _c in _EXTRA:
    ec.CASE_BY_NAME.setdefault(_c.name, _c)

# setter (the fp16 build exports it suffixed _f16) | precisions | case | (value, other value) | where the engine reads it
SWITCHES = [
    ("mivit_mlp_block_bwd_set_waves", ("bf16", "fp16"), "w128_meanpool_late_out3", (4, 8),
     "fused_bwd.hip launch_mlp_block_bwd (g_mlp_bwd_waves), called by engine.hip layer_bwd_fused through FusedOps::mlp_bwd"),
    ("mivit_rowstream_set_wavestream", ("bf16", "fp16"), "w128_gelu_pos_perop_S65", (0, 2),
     "rowstream.hip launch_rowstream (g_use_ws), called by engine.hip lin_fwd / lin_dgrad through StreamOps::rowstream"),
    ("mivit_rowstream_set_wavestream_mask", ("bf16", "fp16"), "w128_gelu_pos_perop_S65", (0, 7),
     "rowstream.hip launch_rowstream (g_ws_mask), same calls"),
    ("mivit_wgrad_bf16_set_config", ("bf16", "fp16"), "w128_gelu_pos_perop_S65", (21, 32),
     "wgrad_dma.hip launch_wgrad_dma (g_cfg), called by engine.hip lin_wgrad through StreamOps::wgrad_dma"),
    ("mivit_embed_set_variant", ("bf16", "fp16"), "w128_P16_embed_dma", (3, 4),
     "embed.hip launch_embed_fwd_dma (g_embed_variant), called by engine.hip's embedding forward through StreamOps::embed_fwd"),
    ("mivit_gemm_dma_set_variant", ("bf16",), "w128_hidden512", (9, 5),
     "gemm_dma.hip launch_variant (g_variant), called by engine.hip lin_fwd / lin_dgrad (bf16 layers the row-stream kernels "
     "do not cover)"),
]


def _native():
    from moleculardiffusion_mivit_amd import _native as N
    return N


# ---- contents -------------------------------------------------------------------------------------------------------------
# x / feats: input salt; labels: 0 = the batch's own, 1 = the same in reverse order; params: 'closed' | 'random'
Contents = namedtuple("Contents", "x feats labels params")


@functools.lru_cache(maxsize=None)
def _params64(name, pset):
    case = ec.CASE_BY_NAME[name]
    closed = orc.closed_form_params(case.cfg, dtype=torch.float64)
    if pset == "closed":
        return closed
    p = {k: v.double() for k, v in orc.random_params(case.cfg, seed=7).items()}
    if case.embedding == "external":          # the tokens of ec.batch come from the closed-form embedding, outside the engine
        p.update({k: v for k, v in closed.items() if k.startswith("embedding.")})
    return p


@functools.lru_cache(maxsize=None)
def _salts(name, B):
    """(a, b): a = pick_salt, admissible under the closed-form parameters; b != a admissible under both parameter sets"""
    case = ec.CASE_BY_NAME[name]
    a = ec.nth_salt(case, B, 0)
    assert a is not None and a == ec.pick_salt(case, B)
    rnd = _params64(name, "random")
    closed = {ec.nth_salt(case, B, n) for n in range(12)}
    b = next((s for s in (ec.nth_salt(case, B, n, rnd) for n in range(12)) if s is not None and s != a and s in closed), None)
    assert b is not None, f"{name} B={B}: no second salt admissible under both parameter sets"
    return a, b


def _tensors(rig, c):
    """the fp32 host tensors of contents `c` for `rig`: x, features, labels, arena"""
    x, labels, _ = ec.batch(rig.case, rig.B, c.x, torch.float32)
    _, _, feats = ec.batch(rig.case, rig.B, c.feats, torch.float32)
    if c.labels:
        labels = labels.flip(0)
    return x.contiguous(), feats, labels.contiguous(), ec.pack_arena(rig.plan, _params64(rig.case.name, c.params))


def load(rig, c, parts=("x", "feats", "labels", "params")):
    """write (parts of) contents `c` into the rig's buffers IN PLACE"""
    x, feats, labels, arena = _tensors(rig, c)
    if "x" in parts:
        rig.x.copy_(x)
    if "feats" in parts and rig.feats is not None:
        rig.feats.copy_(feats)
    if "labels" in parts:
        rig.labels.copy_(labels)
    if "params" in parts:
        rig.arena.copy_(arena)


def _make(name, precision, B=None, c=None):
    case = ec.CASE_BY_NAME[name]
    B = case.batches(precision)[0] if B is None else B
    a, b = _salts(name, B)
    rig = ec.Rig(case, precision, B, a)
    if c is not None:
        load(rig, c)
    return rig, Contents(a, a, 0, "closed"), b


def _fresh_run(name, precision, c, call=None):
    """contents `c` through a new rig: every call is a first sighting, which the counters must show"""
    rig, _, _ = _make(name, precision, c=c)
    torch.cuda.synchronize()
    s0 = stats()
    snap = rig.step(0x00) if call is None else call(rig)
    assert stats() == s0, f"a fresh rig's calls must run directly: counters moved {s0} -> {stats()}"
    return snap


@functools.lru_cache(maxsize=None)
def fresh(name, precision, c):
    """the reference of every comparison, computed once per contents and shared: treat it as read-only"""
    return _fresh_run(name, precision, c)


# ---- one checked step -------------------------------------------------------------------------------------------------------
def _describe(got, ref):
    if got is None or ref is None:
        return "missing" if (got is None) != (ref is None) else None
    if same(got, ref):
        return None
    if bool((bits(got) == ec.SENTINEL).all()):
        return "still holds the sentinel in every word: the call wrote nothing into this buffer"
    n = int((bits(got) != bits(ref)).sum())
    return f"{n} of {got.numel()} words differ from the fresh-rig result ({int((bits(got) == ec.SENTINEL).sum())} hold the sentinel)"


def assert_snap(snap, ref, what, fields=("out", "arena", "dfeat", "dx")):
    bad = {f: d for f in fields for d in [_describe(getattr(snap, f), getattr(ref, f))] if d}
    assert not bad, f"{what}: " + "; ".join(f"{k} {v}" for k, v in bad.items())


def _counted(call, expect, what):
    """one library call; expect 'direct' | 'capture' | 'replay' | None (not asserted).  `failures` must not move."""
    r0, c0, f0 = stats()
    call()
    r1, c1, f1 = stats()
    assert f1 == f0, f"{what}: hipGraph capture failed ({f0} -> {f1})"
    if expect is not None:
        assert (c1 - c0, r1 - r0) == DELTA[expect], \
            f"{what}: expected a {expect} call (captures, replays) += {DELTA[expect]}, counters moved by {(c1 - c0, r1 - r0)}"


def step(rig, fwd, bwd, ref=None, ws_fill=None, what="", **kw):
    """Rig.step (outputs poisoned first, guards checked by the snapshot) with the counters asserted around each library call"""
    _counted(lambda: rig.forward(ws_fill), fwd, f"{what} forward")
    _counted(lambda: rig.backward(**kw), bwd, f"{what} backward")
    snap = rig.snapshot()
    if ref is not None:
        assert_snap(snap, ref, what)
    return snap


def warm(rig, ref, what=""):
    """direct, capture, replay on unchanged contents"""
    return [step(rig, k, k, ref, fill, f"{what} {k}") for k, fill in (("direct", 0x00), ("capture", 0xFF), ("replay", 0x00))]


def fp64_check(rig, snap, salt, what):
    """the comparison of test_accuracy_against_fp64 (closed-form parameters, the batch's own labels), bars unchanged"""
    ref, got = ec.reference(rig.case, rig.B, salt), rig.result(snap)
    assert bool(torch.isfinite(got.out).all())
    if rig.precision == "fp32":
        err = ec.fp32_errors(got, ref)
        worst = max(err, key=err.get)
        print(f"GRAPH-REPLAY {what}: worst fp32 error {worst} {err[worst]:.1e}")
        assert err[worst] < ec.FP32_TOL, (what, worst, err[worst])
    else:
        err, yard = ec.lowp_errors(got, ref), ec.lowp_errors(ec.yardstick(rig.case, rig.B, salt), ref)
        print(f"GRAPH-REPLAY {what}: out {err['out']:.1e} (yardstick {yard['out']:.1e}) loss {err['loss']:.1e} ({yard['loss']:.1e})")
        for k in err:
            assert err[k] <= 3 * yard[k] + ec.lowp_floor(k), (what, k, err[k], yard[k])


# ---- 1. contents change, addresses do not -------------------------------------------------------------------------------------
def a_steps(rig, A, b, first, last, refs=None, counted=True):
    """steps A`first` .. A`last` of section 1 on one rig -> snapshots.  refs: {contents: fresh-rig snapshot} or None"""
    c2 = A._replace(x=b, feats=b)
    c3 = c2._replace(params="random")
    seq = [("A0", A, (), "direct", 0x00), ("A1", A, (), "capture", 0xFF), ("A2", c2, ("x", "feats"), "replay", 0x00),
           ("A3", c3, ("params",), "replay", 0xFF), ("A4", c3._replace(labels=1), ("labels",), "replay", 0x00),
           ("A5", A, ("x", "feats", "labels", "params"), "replay", 0xFF)]
    snaps = []
    for tag, c, parts, kind, fill in seq[first:last + 1]:
        load(rig, c, parts)
        kind = kind if counted else None
        snaps.append(step(rig, kind, kind, None if refs is None else refs[c], fill, f"{tag} {c}"))
    return snaps


@pytest.mark.parametrize("name,precision", GRID, ids=GRID_IDS)
def test_contents_change_at_fixed_addresses(name, precision):
    """What training does: AdamW updates the arena in place, the allocator hands back the same x block, the labels are new.
    A replay must read all of them live."""
    rig, A, b = _make(name, precision)
    cs = [A, A._replace(x=b, feats=b), A._replace(x=b, feats=b, params="random"), A._replace(x=b, feats=b, params="random", labels=1)]
    refs = {c: fresh(name, precision, c) for c in cs}          # (before the rig's keys exist: fresh rigs fill the LRU too)
    assert not same(refs[cs[0]].out, refs[cs[1]].out) and not same(refs[cs[1]].out, refs[cs[2]].out)
    a0, a1 = a_steps(rig, A, b, 0, 1, refs)
    r0, c0, f0 = stats()
    a2, a3, a4, a5 = a_steps(rig, A, b, 2, 5, refs)
    r1, c1, f1 = stats()
    assert (c1 - c0, r1 - r0, f1 - f0) == (0, 8, 0), f"A2..A5: (captures, replays, failures) moved by {(c1 - c0, r1 - r0, f1 - f0)}"
    fp64_check(rig, a2, b, f"{name} {precision} A2 (replay, new x)")
    assert same(a4.out, a3.out), "A4 changed only the labels: its forward result must be A3's"
    assert not same(a4.arena, a3.arena), "A4 changed the labels: its backward result must be new"
    assert_snap(a5, a0, "A5 (everything back to contents A) against A0")
    assert_snap(a1, a0, "A1 against A0")


# ---- 2. one pointer changes at a time -------------------------------------------------------------------------------------------
# pointer argument -> the library calls whose key it is part of
POINTERS = {"params": "fb", "x": "fb", "features": "fb", "workspace": "fb", "out": "f", "dout": "b", "grads": "b",
            "dfeatures": "b", "dx_tokens": "b"}


def _has(case, ptr):
    return {"features": case.cfg.use_global_features, "dfeatures": case.dfeatures, "dx_tokens": case.dx_tokens}.get(ptr, True)


def _poisoned(g):
    return bool((bits(g.t) == ec.SENTINEL).all())


def _swap(rig, ptr, A, b):
    """Put a second buffer in the place of argument `ptr` -> (contents the calls now see, undo, check after the calls).
    The buffer swapped out stays allocated; an output swapped out is poisoned and must keep its sentinel, an input swapped out
    keeps (or, for dout, is given) contents that differ from the new buffer's."""
    c, check = A, (lambda: None)
    if ptr in ("params", "x", "features"):
        attr = {"params": "arena", "x": "x", "features": "feats"}[ptr]
        c = {"params": A._replace(params="random"), "x": A._replace(x=b), "features": A._replace(feats=b)}[ptr]
        old = getattr(rig, attr)
        x, feats, _, arena = _tensors(rig, c)
        setattr(rig, attr, {"params": arena, "x": x, "features": feats}[ptr].cuda())
        assert not same(old, getattr(rig, attr))
    elif ptr == "dout":
        attr, old = "dout", rig.dout
        rig.dout = torch.zeros_like(old)
        old.fill_(float("nan"))                     # (Rig.forward rewrites the buffer in use: a call that reads the old one shows)
    else:
        attr = {"workspace": "ws", "out": "out", "grads": "grads", "dfeatures": "dfeat", "dx_tokens": "dx"}[ptr]
        old = getattr(rig, attr)
        new = ec.Guarded(old.t.numel(), old.t.dtype)
        setattr(rig, attr, new)
        rig.guards = [new if g is old else g for g in rig.guards] + [old]
        if ptr == "workspace":
            def check():
                assert not bool((new.t == 0xFF).all()), "the new workspace was never written: the calls used the old one"
        else:
            bits(old.t).fill_(ec.SENTINEL)

            def check():
                assert _poisoned(old), f"the {ptr} buffer that was swapped out was written"

    def undo():
        setattr(rig, attr, old)
    return c, undo, check


@pytest.mark.parametrize("name,precision,ptr", [(n, p, q) for n, p in GRID for q in POINTERS if _has(ec.CASE_BY_NAME[n], q)],
                         ids=[f"{n}-{p}-{q}" for n, p in GRID for q in POINTERS if _has(ec.CASE_BY_NAME[n], q)])
def test_a_changed_pointer_is_a_new_key(name, precision, ptr):
    """A key that forgot an argument would replay into the old buffer.  After direct / capture / replay, one pointer argument
    is replaced: the calls whose key holds it start over (direct, capture, replay, asserted one by one), the others go on
    replaying; the results are the new buffer's, the old output buffer is not touched, and going back to the first buffer
    replays the first graph."""
    rig, A, b = _make(name, precision)
    cs = {"params": A._replace(params="random"), "x": A._replace(x=b), "features": A._replace(feats=b)}.get(ptr, A)
    refA, ref = fresh(name, precision, A), fresh(name, precision, cs)
    warm(rig, refA, "first buffer")
    c, undo, check = _swap(rig, ptr, A, b)
    assert c == cs
    for kind in ("direct", "capture", "replay"):
        f, bw = (kind if "f" in POINTERS[ptr] else "replay"), (kind if "b" in POINTERS[ptr] else "replay")
        step(rig, f, bw, ref, 0xFF, f"second {ptr} buffer, sighting as {kind}")
        check()
    undo()
    step(rig, "replay", "replay", refA, 0x00, f"back to the first {ptr} buffer")


@pytest.mark.parametrize("name,precision", GRID, ids=GRID_IDS)
def test_need_backward_is_in_the_key(name, precision):
    rig, A, b = _make(name, precision)

    def fwd_only(r, nb=False):
        r._poison()
        r.ws.t.fill_(0xFF)
        r.plan.forward(r.arena, r.x, r.feats, r.B, r.T, r.ws.t, nb, r.out.t)
        torch.cuda.synchronize()
        assert all(g.intact() for g in r.guards), "a kernel wrote outside its buffer"
        return r.out.t.view(r.B, -1).clone()

    ref0 = _fresh_run(name, precision, A, fwd_only)
    refA = fresh(name, precision, A)
    warm(rig, refA, "need_backward = 1")
    for kind in ("direct", "capture", "replay"):
        got = []
        _counted(lambda: got.append(fwd_only(rig)), kind, f"need_backward = 0, sighting as {kind}")
        d = _describe(got[0], ref0)
        assert d is None, f"need_backward = 0, sighting as {kind}: out {d}"
    step(rig, "replay", "replay", refA, 0x00, "back to need_backward = 1")


@pytest.mark.parametrize("name,precision", GRID, ids=GRID_IDS)
def test_stage_range_is_in_the_key(name, precision):
    """backward(s, s + 1) for every stage against backward(0, num_stages): each range is a key of its own"""
    rig, A, b = _make(name, precision)
    refA = fresh(name, precision, A)
    warm(rig, refA, "whole backward")
    n = rig.plan.num_stages
    for kind in ("direct", "capture", "replay"):
        _counted(lambda: rig.forward(0xFF), "replay", "forward")
        for s in range(n):
            _counted(lambda: rig.backward(s, s + 1), kind, f"backward({s}, {s + 1}), sighting as {kind}")
        assert_snap(rig.snapshot(), refA, f"staged backward, sighting as {kind}")
    step(rig, "replay", "replay", refA, 0x00, "back to the whole backward")


# ---- 3. streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", GRID, ids=GRID_IDS)
def test_replay_on_other_streams_is_ordered_on_the_callers_stream(name, precision):
    """The key leaves the stream out on purpose: direct on S1, capture on S2, replay on S3 and on the default stream.  On S3 the
    replay sits between a slow producer, whose last act is to write the real contents over poison, and a consumer that clones
    the results with no host synchronisation in between."""
    rig, A, b = _make(name, precision)
    c2 = A._replace(x=b, feats=b, params="random", labels=1)
    refA, ref2 = fresh(name, precision, A), fresh(name, precision, c2)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for st, kind in ((s1, "direct"), (s2, "capture"), (s3, "replay")):
        with torch.cuda.stream(st):
            step(rig, kind, kind, refA, 0xFF, f"{kind} on a stream of its own")          # (the snapshot synchronises the device)
    # one engine step and one matrix product, timed once with events on S3
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    m = torch.randn(2048, 2048, device="cuda")
    acc = torch.empty_like(m)
    with torch.cuda.stream(s3):
        torch.mm(m, m, out=acc)
        ev[0].record()
        rig.forward()
        rig.backward()
        ev[1].record()
        torch.mm(m, m, out=acc)
        ev[2].record()
        for _ in range(4):
            torch.mm(m, m, out=acc)
        ev[3].record()
    torch.cuda.synchronize()
    t_step, t_mm = ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]) / 4
    links = max(8, math.ceil(20 * t_step / t_mm))
    # the real contents wait on the device; the buffers hold poison
    stage = [t.cuda() for t in _tensors(rig, c2) if t is not None]
    dst = [t for t in (rig.x, rig.feats, rig.labels, rig.arena) if t is not None]
    assert len(stage) == len(dst)
    for t in dst:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    r0, c0, f0 = stats()
    with torch.cuda.stream(s3):
        ev[4].record()
        for _ in range(links):
            torch.mm(m, m, out=acc)
        for d, s in zip(dst, stage):
            d.copy_(s)
        ev[5].record()
        rig.forward(0xFF)
        rig.backward()
        got = {"out": rig.out.t.view(rig.B, -1).clone(), "arena": rig.grads.t.clone(),
               "dfeat": None if rig.dfeat is None else rig.dfeat.t.clone(), "dx": None if rig.dx is None else rig.dx.t.clone()}
    r1, c1, f1 = stats()
    torch.cuda.synchronize()
    t_prod = ev[4].elapsed_time(ev[5])
    msg = f"producer {t_prod:.3f} ms ({links} products of {t_mm:.3f} ms), one engine step {t_step:.3f} ms"
    print(f"GRAPH-REPLAY streams {name} {precision}: {msg}")
    assert t_prod >= 10 * t_step, f"the producer is not slow compared with the call, the ordering check proves nothing: {msg}"
    assert (c1 - c0, r1 - r0, f1 - f0) == (0, 2, 0), (c1 - c0, r1 - r0, f1 - f0)
    assert all(g.intact() for g in rig.guards)
    assert_snap(SimpleNamespace(**got), ref2, f"replay on S3 between producer and consumer ({msg})")
    step(rig, "replay", "replay", ref2, 0x00, "replay on the default stream")


# ---- 4. LRU -------------------------------------------------------------------------------------------------------------------
def test_evicted_key_starts_over():
    """cap + 1 forward-only keys of one rig that differ in `out`: the oldest is evicted, starts over (direct, capture, replay)
    and is still right; a key that was never evicted is captured at its second sighting.  The device is idle at every call:
    this is about bookkeeping."""
    cap = int(os.environ.get("MIVIT_GRAPH_CAP", "32"))
    if cap > 64:
        pytest.skip(f"MIVIT_GRAPH_CAP = {cap}")
    name, precision = "w64_fused_S12", "bf16"
    rig, A, b = _make(name, precision)
    n = rig.B * rig.case.cfg.output_dim
    pitch = (n + 63) // 64 * 64                                  # 256-byte pitch between the keys' outputs

    def fwd_at(r, out):
        r.ws.t.fill_(0xFF)
        r.plan.forward(r.arena, r.x, r.feats, r.B, r.T, r.ws.t, False, out)
        torch.cuda.synchronize()
        return out.clone()

    ref = _fresh_run(name, precision, A, lambda r: fwd_at(r, r.out.t))
    outs = ec.Guarded((cap + 1) * pitch, torch.float32)

    def call(i, kind):
        bits(outs.t).fill_(ec.SENTINEL)
        torch.cuda.synchronize()
        got = []
        _counted(lambda: got.append(fwd_at(rig, outs.t[i * pitch:i * pitch + n])), kind, f"key {i} as {kind}")
        d = _describe(got[0], ref.view(-1))
        assert d is None, f"key {i} as {kind}: out {d}"
        rest = torch.ones(outs.t.numel(), dtype=torch.bool, device="cuda")
        rest[i * pitch:i * pitch + n] = False
        assert bool((bits(outs.t)[rest] == ec.SENTINEL).all()), f"key {i} as {kind}: another key's output was written"
        assert outs.intact() and all(g.intact() for g in rig.guards)

    for i in range(cap + 1):
        call(i, "direct")
    for kind in ("direct", "capture", "replay"):                 # key 0 was the least recently used of cap + 1
        call(0, kind)
    call(cap, "capture")                                         # never evicted: this is its second sighting
    call(cap, "replay")


# ---- 5. DeepResNet training entries ----------------------------------------------------------------------------------------------
DRN_CASE = next(c for c in dc.CASES if c["id"] == "whole-9x9-ragged")


def _drn():
    import test_deepresnet_ops_gpu as T
    return T


# The DeepResNet keys hold pointers and sizes only (no plan uid): a Problem that the allocator places on the blocks of one freed
# earlier would be no first sighting.  Every Problem of this module stays allocated until the module is done.
_KEEP = []


@pytest.fixture(scope="module", autouse=True)
def _release_problems():
    yield
    _KEEP.clear()


def _problem(dt, c):
    _KEEP.append(_drn().Problem(dt, c))
    return _KEEP[-1]


def _drn_fwd(pr, momentum, eps):
    N_, T = _native(), _drn()
    N_.check(N_.lib.mivit_deepresnet_train_fwd(pr.code, ctypes.byref(pr.params), pr.xptr, pr.N, pr.P, pr.E, momentum, eps,
                                               pr.tokens.ptr, pr.ws.data_ptr(), pr.bytes, T._st()), "deepresnet forward")


def _set_x(pr, x):
    R = pr.N * pr.P * pr.P
    pr.xbuf[_drn().GUARD:_drn().GUARD + R] = x.reshape(-1).cuda()
    pr.x64 = x.double().cuda()


def _running(pr):
    torch.cuda.synchronize()
    return [b.raw.clone() for b in pr.rm + pr.rv]


def _seed_running(pr, raws):
    for b, raw in zip(pr.rm + pr.rv, raws):
        b.raw.copy_(raw)
    for i in range(7):
        pr.prm["rm"][i] = pr.rm[i].read().double().clone()
        pr.prm["rv"][i] = pr.rv[i].read().double().clone()


def _same_state(a, b, what):
    (wa, ba), (wb, bb) = a.snapshot(), b.snapshot()
    assert torch.equal(wa, wb), f"{what}: workspace differs from the fresh problem's"
    names = ["tokens", "d fc weight", "d fc bias"] + [f"{k}{i}" for k in ("dW", "dgamma", "dbeta", "running mean ", "running var ") for i in range(7)]
    bad = [n for n, x, y in zip(names, ba, bb) if not torch.equal(x, y)]
    assert not bad, f"{what}: differ from the fresh problem's: {bad}"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_deepresnet_replays_read_live_state(dt):
    """momentum 0.1: the running statistics carry state from call to call, so F2 and F3 are replays whose result depends on what
    the previous replay left behind.  Every call passes the fp64 Walk fed with the running statistics from before the call
    and equals, bitwise, a fresh Problem seeded with the same frames, parameters and pre-call running statistics."""
    T = _drn()
    c = dict(DRN_CASE, momentum=0.1)
    N, P, E = c["N"], c["P"], c["E"]
    assert dc.launch_plan(dt, N, P)["graph"]
    pr = _problem(dt, c)
    kinds = ("direct", "capture", "replay", "replay")
    gf = fw_ref = None
    for k, kind in enumerate(kinds):
        x = dc.make_frames("rand", N, P, 900 + k)
        _set_x(pr, x)
        before = _running(pr)
        _seed_running(pr, before)
        _counted(pr.fwd, kind, f"F{k}")
        gf = pr.got_forward()
        w = dc.Walk(dt, gf)
        dc.walk_forward(w, pr.prm, pr.x64, N, P, E, dc.EPS, pr.momentum, pr.running)
        T._assert(f"replay-F{k}", dt, c["id"], w)
        fp = _problem(dt, c)
        _set_x(fp, x)
        _seed_running(fp, before)
        _counted(fp.fwd, "direct", f"fresh problem for F{k}")
        _same_state(pr, fp, f"F{k} ({kind})")
        assert k == 0 or not torch.equal(_running(pr)[0], before[0]), "the running statistics did not move"
    R = N * P * P
    for k, kind in enumerate(kinds[:3]):
        dtok = torch.randn(N, E, generator=torch.Generator().manual_seed(40 + k))
        pr.dtok.copy_(dtok)
        pr.dtok64 = dtok.double().cuda()
        fp = _problem(dt, c)                          # forward state: F3's frames on the statistics from before F3
        _set_x(fp, x)
        _seed_running(fp, before)
        fp.dtok.copy_(dtok)
        _counted(fp.fwd, "direct", f"fresh problem for B{k}, forward")
        _counted(pr.bwd, kind, f"B{k}")
        gb = pr.got_backward()
        gs = {"g11": pr.region(12, R * 64).reshape(-1, 64), "g0": pr.region(13, R * 32).reshape(-1, 32), "g1": pr.region(14, R * 64).reshape(-1, 64)}
        w = dc.Walk(dt, {**gf, **gs, **gb}, regen=("g2", "g21"))
        fw = dc.walk_forward(w, pr.prm, pr.x64, N, P, E, dc.EPS, pr.momentum, pr.running)
        dc.walk_backward(w, pr.prm, pr.x64, pr.dtok64, fw, N, P, E)
        T._assert(f"replay-B{k}", dt, c["id"], w)
        _counted(fp.bwd, "direct", f"fresh problem for B{k}, backward")
        _same_state(pr, fp, f"B{k} ({kind})")
    pr.check_guard()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["momentum", "eps"])
def test_deepresnet_momentum_eps_in_key(dt, which):
    """only `momentum` or `eps` changes, every pointer stays: a new key, run directly, with the new value's result"""
    T = _drn()
    c = dict(DRN_CASE, momentum=0.1)
    N, P, E = c["N"], c["P"], c["E"]
    pr = _problem(dt, c)
    before = _running(pr)
    for kind in ("direct", "capture", "replay"):
        _seed_running(pr, before)
        _counted(lambda: _drn_fwd(pr, 0.1, dc.EPS), kind, f"momentum 0.1, eps {dc.EPS}: {kind}")
    momentum, eps = (0.37, dc.EPS) if which == "momentum" else (0.1, 3e-3)
    _seed_running(pr, before)
    pr.tokens.raw[_drn().GUARD:_drn().GUARD + pr.tokens.n] = T.SENT
    _counted(lambda: _drn_fwd(pr, momentum, eps), "direct", f"{which} changed")
    w = dc.Walk(dt, pr.got_forward())
    dc.walk_forward(w, pr.prm, pr.x64, N, P, E, eps, momentum, pr.running)
    T._assert(f"new-{which}", dt, c["id"], w)
    fp = _problem(dt, c)
    _seed_running(fp, before)
    _counted(lambda: _drn_fwd(fp, momentum, eps), "direct", "fresh problem")
    _same_state(pr, fp, f"{which} changed")


# ---- 6. switches ----------------------------------------------------------------------------------------------------------------
def _switch_params():
    return [pytest.param(s, p, id=f"{s[0][6:]}-{p}") for s in SWITCHES for p in s[1]]


@pytest.mark.parametrize("switch,precision", _switch_params())
def test_switch_change_starts_the_key_over(switch, precision):
    """After direct / capture / replay under the value in force, the switch changes and the call is repeated with identical
    arguments: it must be a first sighting (a replay would launch the sequence captured under the old value) and give,
    bitwise, what a fresh rig made and run under the new value gives.  With the old value back the result is the old one."""
    setter, _, name, (v1, v1_alt), _where = switch
    fn = getattr(_native().lib, setter + ("_f16" if precision == "fp16" else ""))
    rig, A, b = _make(name, precision)
    ref0 = fresh(name, precision, A)
    warm(rig, ref0, f"{setter} unchanged")
    old = fn(v1)
    try:
        if old == v1:
            fn(v1_alt)
        ref1 = _fresh_run(name, precision, A)
        step(rig, "direct", "direct", ref1, 0xFF, f"after {setter}({v1 if old != v1 else v1_alt}) (was {old})")
    finally:
        fn(old)
    step(rig, None, None, ref0, 0x00, f"{setter} back to {old}")


def _child(outdir):
    """A0 .. A3 of one bf16 case in this process, which was started with MIVIT_GRAPHS=0: no counter may ever move"""
    assert os.environ.get("MIVIT_GRAPHS") == "0" and "MIVIT_GRAPH_CAP" not in os.environ
    rig, A, b = _make(CHILD[0], CHILD[1])
    assert stats() == (0, 0, 0), stats()
    for k, snap in enumerate(a_steps(rig, A, b, 0, 3, counted=False)):
        torch.save({f: getattr(snap, f).cpu() for f in ("out", "arena")}, os.path.join(outdir, f"A{k}.pt"))
        # (the counters never go down: all zero after the last step means all zero before and after each)
    assert stats() == (0, 0, 0), stats()
    print("[graph-replay] child OK")


CHILD = ("w64_fused_S12", "bf16")


def test_graphs_disabled_by_environment(tmp_path):
    """MIVIT_GRAPHS=0 (include/mivit_hip.h): every call runs directly, the counters stay 0, the results are the replayed ones"""
    name, precision = CHILD
    rig, A, b = _make(name, precision)
    snaps = a_steps(rig, A, b, 0, 3)
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MIVIT_GRAPHS="0")
    env.pop("MIVIT_GRAPH_CAP", None)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and "[graph-replay] child OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    for k, snap in enumerate(snaps):
        got = torch.load(os.path.join(str(tmp_path), f"A{k}.pt"))
        for f in ("out", "arena"):
            assert same(got[f], getattr(snap, f).cpu()), f"A{k}: {f} under MIVIT_GRAPHS=0 differs from the run with graphs"


# ---- 7. model level ---------------------------------------------------------------------------------------------------------------
def _raw_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("embedding,precision", [("linear", "bf16"), ("deepresnet", "fp32")])
def test_training_loop_equals_the_unreplayed_loop(embedding, precision):
    """What an experiment loop does -- zero_grad / forward / MSE / backward / AdamW.step on preallocated x and y refilled in
    place -- with graphs active (G) and with the in-library profiler on for the whole loop (D), which include/mivit_hip.h
    documents as bypassing replay.  Loss, out, every parameter and every buffer are bitwise equal after every step."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from util import build_product_model
    N = _native()
    cfg = orc.MiViTConfig(embedding=embedding, patch_size=9, embed_dim=64, num_heads=4, hidden_dim=128, num_layers=2)
    params = orc.random_params(cfg, seed=3)
    sd0 = {k: v.detach().cpu().clone() for k, v in build_product_model(cfg, precision, params).state_dict().items()}

    def loop():
        m = build_product_model(cfg, precision, params).train()
        m.load_state_dict(sd0)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        g = torch.Generator().manual_seed(11)
        x, y = torch.empty(4, 10, 9, 9, device="cuda"), torch.empty(4, 1, device="cuda")
        rec = []
        for _ in range(6):
            x.copy_(torch.rand(4, 10, 9, 9, generator=g))
            y.copy_(torch.rand(4, 1, generator=g))
            opt.zero_grad()
            out = m(x)
            loss = F.mse_loss(out, y)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            r = {"loss": loss.detach().cpu(), "out": out.detach().cpu()}
            r.update({f"state/{k}": v.detach().cpu().clone() for k, v in m.state_dict().items()})
            rec.append(r)                                     # host copies: the device blocks go back to the allocator
            del out, loss
        return rec

    r0, c0, f0 = stats()
    G = loop()
    r1, c1, f1 = stats()
    assert f1 == f0, "hipGraph capture failed during the loop with graphs"
    assert r1 > r0, ("the loop with graphs never replayed: the allocator did not hand back stable addresses (or the model "
                     f"changed an argument every step), so this test compares two unreplayed runs; counters {(r0, c0)} -> {(r1, c1)}")
    counts = []
    try:
        N.check(N.lib.mivit_profile_enable((1 << len(N.PROF_TAGS)) - 1), "profile_enable")
        D = loop()
    finally:
        N.lib.mivit_profile_enable(0)
        for i in range(len(N.PROF_TAGS)):
            ms, n = ctypes.c_double(), ctypes.c_int()
            N.lib.mivit_profile_collect(i, ctypes.byref(ms), ctypes.byref(n))
            counts.append(n.value)
    r2, c2, f2 = stats()
    assert (r2, c2, f2) == (r1, c1, f1), f"the profiled loop must bypass the cache: counters {(r1, c1, f1)} -> {(r2, c2, f2)}"
    assert sum(counts) > 0, "the profiler bracketed no launch"
    for k, (g, d) in enumerate(zip(G, D)):
        assert sorted(g) == sorted(d)
        bad = [key for key in g if not _raw_equal(g[key], d[key])]
        assert not bad, f"step {k}: differ between the loop with graphs and the unreplayed loop: {bad}"
    moved = [k for k in G[0] if k.startswith("state/") and not _raw_equal(G[0][k], G[-1][k])]
    assert moved, "no parameter moved in six steps"


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    _child(sys.argv[2])
