"""GPU: the movie-analysis kernels (tracking.hip, localize.hip, linking.hip, diffusion.hip, segment.hip, hmm.hip, drift.hip,
features.hip) at the C-ABI, inside the guarded, poisoned buffers of tests/abi_guard.py (one call and its checks:
tests/abi_call.py; the generating side of the pipeline: tests/test_simulation_abi_gpu.py).  The numerical suites of these
kernels go through ops.py, whose torch allocations are rounded up, neighbour each other and are pre-zeroed where the header
says "not written"; here every argument is a Buf of exactly the documented size, so the promises of include/mivit_hip.h about
placement and clamping are held to the letter.  Per entry:

  P1 placement    outputs and workspace of exactly the documented size: every guard intact, every entry the header calls "not
                  written" still holds its fill pattern, every other entry holds the host restatement's value (helpers/), under
                  the bar the entry's own suite uses (imported, never copied); one case with every input and output one element
                  off the 256-byte boundary.
  P2 unread       what the header says is not read (slots beyond count[f], rows no track covers, the T % npos trailing
                  sub-steps, the previous contents of an output) is filled with garbage: the result is bitwise that with zeros.
  P3 workspace    the workspace pre-filled with 0xFF, with 0x00 and with the leftovers of a larger problem: bitwise one result.
  P4 clamps       the documented clamps with hostile indices that abi_guard.bounded keeps within the guards: the outputs are the
                  restatement's on the input sanitised on the host as the header sentence says, nothing is poisoned, no guard
                  changed.  Hostile values sit at the ends of a CSR, in reversed pairs at its ends (which empty a track without
                  making two live ranges overlap) and in index slots of single rows.

Integer outputs in which -1 is a legal value start as the GARBAGE pattern, so an unwritten entry cannot pass for a written -1.
Bitwise comparisons treat every NaN as one value (the sign of a computed NaN is the hardware's) and tell -0 from +0.

That these tests can fail was checked on scratch copies of the sources (never committed), each mutation in an entry of its
own, so every failure below belongs to one mutation; what failed, and with which message:
  (a) df_msd_kernel without the `b > N` clamp: test_track_msd_hostile_offsets[ends]: the NaN of the rows past pos reaches msd
      ("still hold the fill pattern": the poison's own bits came through the arithmetic); [reversed] passes, as it should.
  (b) lk_link_kernel not writing -1 for k >= n1: test_link_frames_placement and test_link_frames_hostile_counts at cap 7, 9
      and 65 ("3 / 4 / 32 entries the header says are written still hold the fill pattern"); cap 1 has no such entry.
  (c) mivit_chain_tracks_gaps without the memset of lengths: test_chain_tracks_gaps_placement and _hostile, both caps
      ("lengths: 77 entries ... still hold the fill pattern").
  (d) hmm_estep_kernel with the lanes K .. 7 storing gamma: every hmm test at K = 1, 2 and 3 ("a guard of the output gamma
      changed", or "gamma: 5 entries written that the header says are not written" where the stray lanes hit the rows no track
      covers first); K = 8 passes, as it should.
  (e) mivit_dog_peaks_workspace_bytes 8 bytes short: test_dog_peaks_placement[dog in the workspace] (the last two DoG pixels
      land in the guard), test_dog_peaks_overflow_stays_inside (the last candidate key does), both
      test_dog_peaks_workspace_carries_no_state; [dog returned] placement passes: the last key slot is not used there.
  (f) tk_init_kernel without the reset of the candidate counter: every dog_peaks test (count and n_candidates differ: the
      counter starts from whatever n_candidates held)."""
import functools

import numpy as np
import pytest
import torch

import abi_guard as G
import hmm_common as hc
import localize_common as LC
import segment_common as sc
import tracking_common as tc
import trajfeat_common as tf
from abi_call import POISON64, Call, bits_equal, check_all, expect, same_results, sanitise_csr
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as M
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

F64, F32, I32, U8 = torch.float64, torch.float32, torch.int32, torch.uint8
GARBAGE32 = 0x3A3A3A3A


def covered(pairs, n):
    m = np.zeros(n, bool)
    for a, b in pairs:
        assert not m[a:b].any(), "two live ranges overlap: the header does not define that"
        m[a:b] = True
    return m


def table(lengths, seed, lead=0, tail=0, scale=0.6):
    """Brownian tracks of the given rows, stacked, with `lead` / `tail` rows that no track covers -> (pos [N, 2], offsets)"""
    rng = np.random.default_rng(seed)
    tracks = [np.cumsum(rng.standard_normal((L, 2)) * scale, axis=0) + 20.0 for L in lengths]
    pos = np.concatenate([np.zeros((lead, 2))] + tracks + [np.zeros((tail, 2))], axis=0)
    offsets = lead + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.ascontiguousarray(pos), offsets


def hostile_csr(offsets, n, row_bytes, kind):
    """"ends": the first offset below 0 and the last above n (only where they were 0 and n: the tracks keep their rows);
    "reversed": the first pair and the last pair reversed, which empties the first and the last track."""
    raw = np.array(offsets, np.int64)
    if kind == "ends":
        assert raw[0] == 0 and raw[-1] == n
        raw[0], raw[-1] = -3, n + 2
    else:
        raw[0] = raw[1] + 2
        raw[-1] = raw[-2] - 3
    return G.bounded(raw, 0, n, row_bytes)


def with_unread(pos, unread, value):
    p = pos.copy()
    p[unread] = value
    return p


# ----------------------------------------------------------------------------------------------------------------------
# mivit_track_msd
# ----------------------------------------------------------------------------------------------------------------------
MSD_LENGTHS = (3, 0, 257, 1, 2)
MSD_DT = 0.5


def msd_call(pos, raw, Lmax, max_lag=0, mis=0):
    c = Call("mivit_track_msd", mis)
    n_tracks = len(raw) - 1
    c.run(c.inp("pos", pos, F64), len(pos), c.inp("offsets", raw, I32), n_tracks, MSD_DT, max_lag, Lmax,
          c.out("msd", (n_tracks, Lmax), F64), c.out("d_lstsq", n_tracks, F64), c.out("d_weighted", n_tracks, F64))
    return c


def msd_ref(pos, pairs, Lmax, max_lag=0):
    """the restatement track by track; "lags beyond Lmax - 1 are not computed" is max_lag = Lmax - 1"""
    eff = Lmax - 1 if max_lag == 0 else min(max_lag, Lmax - 1)
    msd, dl, dw = np.zeros((len(pairs), Lmax)), np.full(len(pairs), np.nan), np.full(len(pairs), np.nan)
    for k, (a, b) in enumerate(pairs):
        if b - a >= 2 and eff >= 1:
            m, l, w = M._track_msd_numpy(pos[a:b], np.array([0, b - a]), MSD_DT, eff)
            msd[k, :min(Lmax, m.shape[1])] = m[0, :Lmax]
            dl[k], dw[k] = l[0], w[0]
    return {"msd": msd, "d_lstsq": dl, "d_weighted": dw}


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("Lmax,max_lag", [(257, 0), (5, 0), (257, 3)])
def test_track_msd_placement(Lmax, max_lag, mis):
    pos, off = table(MSD_LENGTHS, 1)
    c = msd_call(pos, off, Lmax, max_lag, mis)
    check_all(c, msd_ref(pos, sanitise_csr(off, len(pos)), Lmax, max_lag))


def test_track_msd_reads_no_row_outside_the_tracks():
    pos, off = table(MSD_LENGTHS, 2, lead=2, tail=3)
    unread = ~covered(sanitise_csr(off, len(pos)), len(pos))
    a = msd_call(with_unread(pos, unread, POISON64), off, 257)
    b = msd_call(with_unread(pos, unread, 0.0), off, 257)
    same_results(a, b)
    check_all(a, msd_ref(pos, sanitise_csr(off, len(pos)), 257))


@pytest.mark.parametrize("kind", ["ends", "reversed"])
def test_track_msd_hostile_offsets(kind):
    pos, off = table(MSD_LENGTHS, 3)
    raw = hostile_csr(off, len(pos), 16, kind)
    pairs = sanitise_csr(raw, len(pos))
    unread = ~covered(pairs, len(pos))
    c = msd_call(with_unread(pos, unread, POISON64), raw, 257)
    check_all(c, msd_ref(pos, pairs, 257))


# ----------------------------------------------------------------------------------------------------------------------
# mivit_segment_tracks, mivit_segment_stats, mivit_markov_states
# ----------------------------------------------------------------------------------------------------------------------
SEG_LENGTHS = (5, 0, 70, 1, 9, 2)


def seg_table(seed, lead=0, tail=0):
    """SEG_LENGTHS, the 70-row track with a planted change of its step variance after 35 increments"""
    pos, off = table(SEG_LENGTHS, seed, lead, tail, scale=0.3)
    a = int(off[2])
    steps = np.random.default_rng(seed + 100).standard_normal((69, 2)) * np.where(np.arange(69) < 35, 0.3, 3.0)[:, None]
    pos[a + 1:a + 70] = pos[a] + np.cumsum(steps, axis=0)
    return pos, off


def seg_call(pos, raw, max_len, min_len, mis=0):
    c = Call("mivit_segment_tracks", mis)
    n_tracks = len(raw) - 1
    c.run(c.inp("pos", pos, F64), len(pos), c.inp("offsets", raw, I32), n_tracks, max_len, min_len, sc.PENALTY, sc.MIN_VAR,
          c.out("seg_start", len(pos), I32), c.out("cost", n_tracks, F64))
    return c


def seg_ref(pos, pairs, min_len):
    """-> (want, written): the restatement track by track; the partition may be compared exactly only where the chosen
    candidates lead the runners-up by segment_common.MIN_MARGIN, which is asserted (a property of the input)"""
    seg, cost = np.zeros(len(pos), np.int32), np.full(len(pairs), np.nan)
    for k, (a, b) in enumerate(pairs):
        if b > a:
            s, c, margin = M._segment_numpy(pos[a:b], np.array([0, b - a]), min_len, sc.PENALTY, sc.MIN_VAR, return_margin=True)
            assert margin[0] >= sc.MIN_MARGIN
            seg[a:b], cost[k] = s, c[0]
    return {"seg_start": seg, "cost": cost}, {"seg_start": covered(pairs, len(pos))}


def seg_cost_close(got, want, what):
    """the bar of tests/test_segment_gpu.py: COST_RTOL (1 + |cost|), NaN where the restatement has NaN"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= sc.COST_RTOL * (1 + np.abs(want[ok]))).all(), (what, got, want)


SEG_CLOSE = {"cost": seg_cost_close}


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("min_len", [2, 4])
def test_segment_tracks_placement(min_len, mis):
    pos, off = seg_table(4, lead=2, tail=3)
    pairs = sanitise_csr(off, len(pos))
    unread = ~covered(pairs, len(pos))
    a = seg_call(with_unread(pos, unread, POISON64), off, 70, min_len, mis)
    want, written = seg_ref(pos, pairs, min_len)
    assert want["seg_start"].sum() > sum(L > 0 for L in SEG_LENGTHS), "the planted changepoint was not found"
    check_all(a, want, written, SEG_CLOSE)
    b = seg_call(with_unread(pos, unread, 0.0), off, 70, min_len, mis)
    same_results(a, b)


@pytest.mark.parametrize("kind", ["ends", "reversed", "max_len"])
def test_segment_tracks_hostile(kind):
    pos, off = seg_table(5)
    n = len(pos)
    if kind == "max_len":                                                 # understated by one: the 70-row track is cut to 69
        raw, max_len = G.bounded(off, 0, n, 16), 69
        pairs = [(a, min(b, a + 69)) for a, b in sanitise_csr(raw, n)]
    else:
        raw, max_len = hostile_csr(off, n, 16, kind), 70
        pairs = sanitise_csr(raw, n)
    c = seg_call(with_unread(pos, ~covered(pairs, n), POISON64), raw, max_len, 4)
    want, written = seg_ref(pos, pairs, 4)
    check_all(c, want, written, SEG_CLOSE)


def stats_case(n_seg, seed):
    """segments of 0 .. 6 rows; half of them end their track (n = rows - 1), the others bridge to the next (n = rows)"""
    rng = np.random.default_rng(seed)
    rows = rng.choice([0, 1, 2, 3, 6], n_seg)
    rows[:min(n_seg, 3)] = [3, 1, 2][:min(n_seg, 3)]
    seg_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    n = int(seg_off[-1])
    end = np.where(rng.random(n_seg) < 0.5, seg_off[1:], np.minimum(seg_off[1:] + 3, n))
    end[-1] = n
    pos = np.cumsum(rng.standard_normal((n, 2)), axis=0)
    return pos, seg_off, end.astype(np.int64)


def stats_call(pos, seg_off, end, mis=0):
    c = Call("mivit_segment_stats", mis)
    n_seg = len(end)
    c.run(c.inp("pos", pos, F64), len(pos), c.inp("seg_offsets", seg_off, I32), c.inp("seg_track_end", end, I32), n_seg, 0.25,
          0.1, c.out("d_cve", n_seg, F64), c.out("d_mle", n_seg, F64), c.out("sigma2", n_seg, F64),
          c.out("n_increments", n_seg, I32))
    return c


def stats_ref(pos, seg_off, end):
    return dict(zip(("d_cve", "d_mle", "sigma2", "n_increments"), M._segment_stats_numpy(pos, seg_off, end, 0.25, 0.1)))


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n_seg", [1, 257])
def test_segment_stats_placement(n_seg, mis):
    pos, seg_off, end = stats_case(n_seg, 6)
    want = stats_ref(pos, seg_off, end)
    if n_seg > 1:
        assert {0, 1, 2} <= set(want["n_increments"].tolist())
    check_all(stats_call(pos, seg_off, end, mis), want)


@pytest.mark.parametrize("n_seg", [1, 257])
def test_segment_stats_hostile(n_seg):
    pos, seg_off, end = stats_case(n_seg, 7)
    n = len(pos)
    seg_off, end = seg_off.copy(), end.copy()
    seg_off[0], seg_off[-1], end[-1] = -2, n + 2, n + 3
    if n_seg > 1:
        end[5], end[9] = -1, n + 2                                        # index slots of single rows
        seg_off[20], seg_off[21] = seg_off[21], seg_off[20]               # a reversed pair: no increments
        seg_off[40] = -3
    raw_off, raw_end = G.bounded(seg_off, 0, n, 16), G.bounded(end, 0, n, 16)
    clean = np.maximum(raw_off.astype(np.int64), 0)                       # "rows are clamped to [0, N - 1]": r0 from below, r1 from above
    check_all(stats_call(pos, raw_off, raw_end), stats_ref(pos, clean, raw_end.astype(np.int64)))


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("n", [1, 65])
def test_markov_states_placement(n, steps, K, mis):
    rng = np.random.default_rng(8)
    u = rng.random((n, steps))
    p0 = rng.dirichlet(np.ones(K))
    Mx = rng.dirichlet(np.ones(K), size=K)
    c = Call("mivit_markov_states", mis)
    c.run(c.inp("u", u, F64), c.inp("p0", p0, F64), c.inp("M", Mx, F64), n, steps, K, c.out("state", (n, steps), I32))
    expect(c, "state", gen._markov_host(u, p0, Mx))


# ----------------------------------------------------------------------------------------------------------------------
# mivit_hmm_estep, mivit_hmm_viterbi
# ----------------------------------------------------------------------------------------------------------------------
HMM_LENGTHS = (3, 0, 40, 1, 2, 40, 2, 3, 1)
HMM_STATS = ("xi", "g_sum", "gq_sum", "g_first", "loglik")


def hmm_table(n_tracks, seed, lead=0, tail=0):
    lengths = HMM_LENGTHS[:n_tracks] if n_tracks > 1 else (40,)
    rng = np.random.default_rng(seed)
    tracks = [hc.switching_track(rng, L, hc.DS3, hc.M3)[0] if L else np.zeros((0, 2)) for L in lengths]
    pos = np.concatenate([np.zeros((lead, 2))] + tracks + [np.zeros((tail, 2))], axis=0)
    return np.ascontiguousarray(pos), lead + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def estep_call(pos, raw, v, A, pi, mis=0, ws_fill=G.POISON):
    c = Call("mivit_hmm_estep", mis)
    n, nt, K = len(pos), len(raw) - 1, len(v)
    ws = c.work(n * K * 8, F64, ws_fill)
    c.run(c.inp("pos", pos, F64), n, c.inp("offsets", raw, I32), nt, K, c.inp("v", v, F64), c.inp("A", A, F64),
          c.inp("pi", pi, F64), c.out("gamma", (n, K), F64), c.out("state", n, I32), c.out("xi", (nt, K, K), F64),
          c.out("g_sum", (nt, K), F64), c.out("gq_sum", (nt, K), F64), c.out("g_first", (nt, K), F64), c.out("loglik", nt, F64),
          ws)
    return c


def viterbi_call(pos, raw, v, A, pi, mis=0, ws_fill=G.POISON):
    c = Call("mivit_hmm_viterbi", mis)
    n, nt, K = len(pos), len(raw) - 1, len(v)
    with np.errstate(divide="ignore"):
        logs = np.log(v), np.log(A), np.log(pi)
    ws = c.work(n * 8, U8, ws_fill)
    c.run(c.inp("pos", pos, F64), n, c.inp("offsets", raw, I32), nt, K, c.inp("v", v, F64), c.inp("logv", logs[0], F64),
          c.inp("logA", logs[1], F64), c.inp("logpi", logs[2], F64), c.out("state", n, I32), c.out("logp", nt, F64), ws)
    return c, logs


def hmm_ref(pos, pairs, v, A, pi, logs):
    """both restatements track by track -> (estep want, viterbi want, written masks of the per-row outputs)"""
    n, nt, K = len(pos), len(pairs), len(v)
    e = {"gamma": np.zeros((n, K)), "state": np.zeros(n, np.int32), "xi": np.zeros((nt, K, K)), "g_sum": np.zeros((nt, K)),
         "gq_sum": np.zeros((nt, K)), "g_first": np.zeros((nt, K)), "loglik": np.zeros(nt)}
    vit = {"state": np.zeros(n, np.int32), "logp": np.zeros(nt)}
    for k, (a, b) in enumerate(pairs):
        one = np.array([0, b - a])
        g, s, xi, gs, gq, gf, ll = M._hmm_estep_numpy(pos[a:b], one, v, A, pi)
        e["gamma"][a:b], e["state"][a:b] = g, s
        e["xi"][k], e["g_sum"][k], e["gq_sum"][k], e["g_first"][k], e["loglik"][k] = xi[0], gs[0], gq[0], gf[0], ll[0]
        if K > 1 and b - a >= 2 and np.isfinite(g).all():                # the state may be compared on every row (hmm_common)
            top = np.sort(g, axis=1)
            assert (top[:, -1] - top[:, -2]).min() >= hc.MIN_GAP
        s, lp = M._hmm_viterbi_numpy(pos[a:b], one, v, *logs)
        vit["state"][a:b], vit["logp"][k] = s, lp[0]
    rows = covered(pairs, n)
    return e, vit, rows


def gamma_close(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= hc.HMM_TOL).all(), (what, float(np.abs(got[ok] - want[ok]).max()))


def stat_close(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), what
    fin = np.isfinite(want)
    hc.close(got[fin], want[fin], what)


ESTEP_CLOSE = dict({"gamma": gamma_close}, **{s: stat_close for s in HMM_STATS})


def check_hmm(ce, cv, e, vit, rows):
    check_all(ce, e, {"gamma": rows[:, None], "state": rows}, ESTEP_CLOSE)
    check_all(cv, vit, {"state": rows})


# the misaligned case once per K, on the largest batch
@pytest.mark.parametrize("name,n_tracks,mis", [(k, n, 0) for k in ("K1", "K3", "K8") for n in (1, 8, 9)]
                         + [(k, 9, 1) for k in ("K1", "K3", "K8")])
def test_hmm_placement(name, n_tracks, mis):
    v, A, pi = hc.parameter_sets()[name]
    pos, off = hmm_table(n_tracks, 9, lead=2, tail=3)
    pairs = sanitise_csr(off, len(pos))
    unread = ~covered(pairs, len(pos))
    ce = estep_call(with_unread(pos, unread, POISON64), off, v, A, pi, mis)
    cv, logs = viterbi_call(with_unread(pos, unread, POISON64), off, v, A, pi, mis)
    check_hmm(ce, cv, *hmm_ref(pos, pairs, v, A, pi, logs))
    same_results(ce, estep_call(with_unread(pos, unread, 0.0), off, v, A, pi, mis))
    same_results(cv, viterbi_call(with_unread(pos, unread, 0.0), off, v, A, pi, mis)[0])


def test_hmm_workspace_carries_no_state():
    v, A, pi = hc.parameter_sets()["K3"]
    pos, off = hmm_table(9, 10)
    big_pos, big_off = hmm_table(9, 11, tail=40)                          # a larger problem: its leftovers fill the buffer
    big_e = estep_call(big_pos, big_off, v, A, pi)
    big_v = viterbi_call(big_pos, big_off, v, A, pi)[0]
    ne, nv = len(pos) * 3 * 8, len(pos) * 8
    first_e, first_v = estep_call(pos, off, v, A, pi, ws_fill=0xFF), viterbi_call(pos, off, v, A, pi, ws_fill=0xFF)[0]
    for fe, fv in ((0x00, 0x00), (big_e.ws.body_bytes()[:ne].view(F64), big_v.ws.body_bytes()[:nv])):
        same_results(first_e, estep_call(pos, off, v, A, pi, ws_fill=fe))
        same_results(first_v, viterbi_call(pos, off, v, A, pi, ws_fill=fv)[0])


@pytest.mark.parametrize("kind", ["ends", "reversed"])
def test_hmm_hostile_offsets(kind):
    v, A, pi = hc.parameter_sets()["K3"]
    pos, off = hmm_table(9, 12)
    raw = hostile_csr(off, len(pos), 8 * 8, kind)                         # the widest row an offset indexes: gamma [N, 8] would be 64 B
    pairs = sanitise_csr(raw, len(pos))
    unread = ~covered(pairs, len(pos))
    ce = estep_call(with_unread(pos, unread, POISON64), raw, v, A, pi)
    cv, logs = viterbi_call(with_unread(pos, unread, POISON64), raw, v, A, pi)
    check_hmm(ce, cv, *hmm_ref(pos, pairs, v, A, pi, logs))


def test_hmm_underflow_and_nan_rows_stay_on_their_track():
    v, A, _ = hc.parameter_sets()["K2_identity"]
    pi = np.array([1.0, 0.0])                                             # the narrow state only: a large step is impossible
    pos, off = hmm_table(9, 13)
    pairs = sanitise_csr(off, len(pos))
    bad = pos.copy()
    a, b = pairs[2]
    bad[a + 10:b, 0] += np.sqrt(1e4 * hc.V_WIDEST)                        # track 2 underflows at its increment 9
    a5, b5 = pairs[5]
    bad[a5 + 7] = np.nan                                                  # track 5 has a NaN row
    ce, (cv, logs) = estep_call(bad, off, v, A, pi), viterbi_call(bad, off, v, A, pi)
    e, vit, rows = hmm_ref(bad, pairs, v, A, pi, logs)
    assert e["loglik"][2] == -np.inf and np.isnan(e["loglik"][5]) and np.isnan(e["gamma"][a5:b5]).all()
    check_hmm(ce, cv, e, vit, rows)
    clean_e, clean_v = estep_call(pos, off, v, A, pi), viterbi_call(pos, off, v, A, pi)[0]
    keep_rows = np.ones(len(pos), bool)
    keep_rows[a:b] = keep_rows[a5:b5] = False
    keep_tracks = np.array([k not in (2, 5) for k in range(9)])
    for got, clean in ((ce, clean_e), (cv, clean_v)):
        for name in got.outs:
            g, c = got.outs[name].numpy(), clean.outs[name].numpy()
            keep = keep_rows if len(g) == len(pos) else keep_tracks
            assert bits_equal(g[keep], c[keep]), name


# ----------------------------------------------------------------------------------------------------------------------
# mivit_drift_frames, mivit_drift_integrate
# ----------------------------------------------------------------------------------------------------------------------
DRIFT_PAIRS = (3, 0, 257, 1, 2)
DRIFT_ROWS = 300


def drift_case(seed, lead=0, tail=0):
    """-> (pos [300, 2], pair_row [lead + 263 + tail] with garbage in the slots no frame covers, frame_offsets [6])"""
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.standard_normal((DRIFT_ROWS, 2)), axis=0)
    m = sum(DRIFT_PAIRS)
    pair_row = np.concatenate([np.full(lead, GARBAGE32), rng.integers(1, DRIFT_ROWS, m), np.full(tail, GARBAGE32)])
    return pos, pair_row.astype(np.int64), lead + np.concatenate([[0], np.cumsum(DRIFT_PAIRS)]).astype(np.int64)


def drift_call(pos, pair_row, raw, mode, max_pairs=257, mis=0):
    c = Call("mivit_drift_frames", mis)
    F = len(raw) - 1
    c.run(c.inp("pos", pos, F64), len(pos), c.inp("pair_row", pair_row, I32), len(pair_row), c.inp("frame_offsets", raw, I32), F,
          mode, max_pairs, c.out("stat", (F, 2), F64))
    return c


def drift_ref(pos, pair_row, pairs, mode, cut=None):
    """the restatement frame by frame on the rows clamped to [1, N - 1]; cut: the pairs a frame keeps (the median's LDS)"""
    stat = np.zeros((len(pairs), 2))
    rows = np.clip(pair_row, 1, len(pos) - 1)
    for f, (a, b) in enumerate(pairs):
        b = b if cut is None else min(b, a + cut)
        stat[f] = M._drift_frames_numpy(pos, rows[a:b], np.array([0, b - a]), mode)[0]
    return {"stat": stat}


def drift_unread(pos, pair_row, pairs):
    used = np.zeros(len(pos), bool)
    for a, b in pairs:
        r = np.clip(pair_row[a:b], 1, len(pos) - 1)
        used[r] = used[r - 1] = True
    return ~used


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_drift_frames_placement(mode, mis):
    pos, pair_row, off = drift_case(14, lead=2, tail=3)
    pairs = sanitise_csr(off, len(pair_row))
    unread = drift_unread(pos, pair_row, pairs)
    assert unread.any()
    a = drift_call(with_unread(pos, unread, POISON64), pair_row, off, mode, mis=mis)
    check_all(a, drift_ref(pos, pair_row, pairs, mode))
    zeroed = pair_row.copy()
    zeroed[~covered(pairs, len(pair_row))] = 0
    same_results(a, drift_call(with_unread(pos, unread, 0.0), zeroed, off, mode, mis=mis))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["ends", "reversed"])
def test_drift_frames_hostile(kind, mode):
    pos, pair_row, off = drift_case(15)
    n, m = len(pos), len(pair_row)
    raw = hostile_csr(off, m, 4, kind)
    pair_row = pair_row.copy()
    pair_row[[0, 4, 100, 262]] = [0, -3, n, n + 2]                        # index slots of single rows, one in every frame size
    raw_rows = G.bounded(pair_row, 1, n - 1, 16)
    pairs = sanitise_csr(raw, m)
    c = drift_call(with_unread(pos, drift_unread(pos, pair_row, pairs), POISON64), raw_rows, raw, mode)
    check_all(c, drift_ref(pos, pair_row, pairs, mode))


def test_drift_frames_median_cuts_a_frame_to_the_lds_of_the_launch():
    pos, pair_row, off = drift_case(16)
    pairs = sanitise_csr(off, len(pair_row))
    c = drift_call(pos, pair_row, off, 1, max_pairs=256)                  # understated by one: 256 pairs of LDS, frame 2 has 257
    check_all(c, drift_ref(pos, pair_row, pairs, 1, cut=256))
    assert not bits_equal(c.outs["stat"].numpy(), drift_ref(pos, pair_row, pairs, 1)["stat"]), "the cut changes this median"


def integrate_case(F, seed):
    rng = np.random.default_rng(seed)
    n_pairs = rng.integers(0, 6, F).astype(np.int64)
    stat = np.where(n_pairs[:, None] > 0, rng.standard_normal((F, 2)), 0.0)
    return stat, n_pairs


def integrate_call(stat, n_pairs, h, mis=0):
    c = Call("mivit_drift_integrate", mis)
    F = len(stat)
    c.run(c.inp("stat", stat, F64), c.inp("n_pairs", n_pairs, I32), F, h, c.out("velocity", (F, 2), F64),
          c.out("drift", (F, 2), F64))
    return c


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("F", [1, 2, 257, 513])
def test_drift_integrate_placement_and_clamps(F, mis):
    stat, n_pairs = integrate_case(F, 17)
    hostile = n_pairs.copy()
    hostile[::5] = -hostile[::5] - 1                                      # negative counts as 0
    stat_h = stat.copy()
    stat_h[::5] = 3.25                                                    # ... whatever the statistic of such a frame holds
    for h in (0, 2, F + 5):
        want = dict(zip(("velocity", "drift"), M._drift_integrate_numpy(stat, n_pairs, min(h, F))))
        check_all(integrate_call(stat, n_pairs, h, mis), want)
        clean = np.maximum(hostile, 0)
        want = dict(zip(("velocity", "drift"), M._drift_integrate_numpy(stat_h, clean, min(h, F))))
        check_all(integrate_call(stat_h, hostile, h, mis), want)


# ----------------------------------------------------------------------------------------------------------------------
# mivit_track_sequences
# ----------------------------------------------------------------------------------------------------------------------
SEQ_MOVIE = (4, 9, 11)
SEQ_ROWS = 12


def seq_case(seed):
    rng = np.random.default_rng(seed)
    F, H, W = SEQ_MOVIE
    movie = rng.uniform(1.0, 100.0, SEQ_MOVIE).astype(np.float32)
    frame = rng.integers(0, F, SEQ_ROWS)
    y, x = rng.integers(0, H, SEQ_ROWS), rng.integers(0, W, SEQ_ROWS)     # P = 3, 5: many patches hang over the border
    y[:4], x[:4] = [0, H - 1, 0, H - 1], [0, W - 1, W - 1, 0]             # the four corners: half the patch is outside
    return movie, frame, y, x


def seq_call(movie, frame, y, x, seq_row, steps, P, normalize, mis=0):
    c = Call("mivit_track_sequences", mis)
    F, H, W = movie.shape
    c.run(c.inp("movie", movie, F32), F, H, W, c.inp("frame", frame, I32), c.inp("y", y, I32), c.inp("x", x, I32), len(frame),
          c.inp("seq_row", seq_row, I32), len(seq_row), steps, P, 7.5, 90.25, normalize,
          c.out("seq", (len(seq_row), steps, P, P), F32))
    return c


def seq_ref(movie, frame, y, x, seq_row, steps, P, normalize):
    """helpers/tracking.track_sequences' host arithmetic on given window starts; a row outside [0, N) or a frame outside
    [0, F) gives a zero patch"""
    rows = (np.asarray(seq_row, np.int64)[:, None] + np.arange(steps)[None, :]).reshape(-1)
    live = (rows >= 0) & (rows < len(frame))
    r = np.where(live, rows, 0)
    fr = np.asarray(frame, np.int64)[r]
    live &= (fr >= 0) & (fr < movie.shape[0])
    patches = T.extract_patches_flat(torch.from_numpy(movie), np.where(live, fr, 0), np.asarray(y)[r], np.asarray(x)[r], P)
    if normalize:
        patches = (patches - 7.5) / 90.25
    patches = torch.where(torch.from_numpy(live)[:, None, None], patches, torch.zeros((), dtype=patches.dtype))
    return {"seq": patches.reshape(len(seq_row), steps, P, P).numpy()}


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n_seq,steps,P", [(3, 2, 3), (5, 3, 5)])
def test_track_sequences_placement(n_seq, steps, P, normalize, mis):
    movie, frame, y, x = seq_case(18)
    seq_row = np.arange(n_seq) * 2                                        # windows overlap and start at the four corner rows
    c = seq_call(movie, frame, y, x, seq_row, steps, P, normalize, mis)
    check_all(c, seq_ref(movie, frame, y, x, seq_row, steps, P, normalize))


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n_seq,steps,P", [(3, 2, 3), (5, 3, 5)])
def test_track_sequences_hostile(n_seq, steps, P, normalize):
    movie, frame, y, x = seq_case(19)
    F, H, W = SEQ_MOVIE
    n = SEQ_ROWS
    seq_row = np.array([-1, n - 1, 3, -steps, n][:n_seq])                 # windows that start before row 0 and run past N
    frame = frame.copy()
    frame[[0, 4, 7]] = [-1, F, F + 1]
    y, x = y.copy(), x.copy()
    y[5], x[5], y[1], x[1] = -2, 3, H + 1, W + 1                          # centres outside the frame: the patch is (nearly) all zeros
    # a frame index moves the access by a whole frame (396 B), y by a line, x and seq_row by an element
    c = seq_call(movie, G.bounded(frame, 0, F - 1, H * W * 4), G.bounded(y, 0, H - 1, W * 4),
                 G.bounded(x, 0, W - 1, 4), G.bounded(seq_row, 0, n - 1, 4), steps, P, normalize)
    check_all(c, seq_ref(movie, frame, y, x, seq_row, steps, P, normalize))


# ----------------------------------------------------------------------------------------------------------------------
# mivit_link_frames, mivit_close_gaps, mivit_chain_tracks, mivit_chain_tracks_gaps
# ----------------------------------------------------------------------------------------------------------------------
LINK_DISTANCE = 15.0


def scene(cap, F, seed, counts=None, p_dark=0.3, dark_frame=None):
    """cap particles on slow lattice walks; frame f shows a subset of them in shuffled order (counts[f] of them, or each with
    probability 1 - p_dark; all of them in frame 0, none in dark_frame) -> (coords [F, cap, 2] with GARBAGE beyond the
    count, counts [F], who: per frame the particle of every detection)."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, 40 + 12 * cap, (1, cap, 2)) + np.cumsum(rng.integers(-2, 3, (F, cap, 2)), axis=0)
    coords = np.full((F, cap, 2), GARBAGE32, np.int64)
    who = []
    for f in range(F):
        if counts is not None:
            ids = rng.permutation(cap)[:counts[f]]
        else:
            vis = (rng.random(cap) > p_dark) | (f == 0)
            ids = rng.permutation(np.flatnonzero(vis & (f != dark_frame)))
        coords[f, :len(ids)] = pos[f, ids]
        who.append(ids)
    return coords, np.array([len(w) for w in who], np.int64), who


def links_of(who, cap, max_gap):
    """the links a perfect tracker would give -> (link, gap_partner, gap_frames) [F, cap], GARBAGE beyond the count"""
    F = len(who)
    link, gp, gf = (np.full((F, cap), GARBAGE32, np.int64) for _ in range(3))
    where = [{int(p): j for j, p in enumerate(w)} for w in who]
    for f in range(F):
        for j, p in enumerate(who[f]):
            link[f, j], gp[f, j], gf[f, j] = -1, -1, 0
            if f > 0 and int(p) in where[f - 1]:
                link[f, j] = where[f - 1][int(p)]
                continue
            for g in range(2, max_gap + 2):
                if f - g >= 0 and int(p) in where[f - g]:
                    gp[f, j], gf[f, j] = where[f - g][int(p)], g
                    break
    return link, gp, gf


def clean_counts(counts, cap):
    return np.clip(np.asarray(counts, np.int64), 0, cap).astype(np.int32)


def clean_links(link, counts):
    """a value outside 0 .. count[f - 1] - 1 counts as -1; slots beyond count[f] are -1 (never read)"""
    out = np.full(link.shape, -1, np.int32)
    for f in range(1, len(link)):
        l = link[f, :counts[f]]
        out[f, :counts[f]] = np.where((l >= 0) & (l < counts[f - 1]), l, -1)
    return out


def clean_gaps(gp, gf, counts, max_gap):
    """a g outside 2 .. max_gap + 1 or beyond frame 0, or a partner outside the partner frame's count, counts as absent"""
    p_out, g_out = np.full(gp.shape, -1, np.int32), np.zeros(gf.shape, np.int32)
    for f in range(len(gp)):
        for j in range(counts[f]):
            g, p = int(gf[f, j]), int(gp[f, j])
            if 2 <= g <= max_gap + 1 and f - g >= 0 and 0 <= p < counts[f - g]:
                p_out[f, j], g_out[f, j] = p, g
    return p_out, g_out


def zero_beyond(a, counts):
    a = a.copy()
    for f in range(len(a)):
        a[f, max(int(counts[f]), 0):] = 0
    return a


def beyond(counts, cap):
    return np.arange(cap)[None, :] >= np.asarray(counts)[:, None]


def ms_bool(ms):
    return None if ms is None else np.asarray(ms) != 0


def link_call(coords, counts, ms, mis=0):
    c = Call("mivit_link_frames", mis)
    F, cap = coords.shape[:2]
    c.run(c.inp("coords", coords, I32), c.inp("count", counts, I32), c.inp("movie_start", ms, U8) if ms is not None else None,
          F, cap, LINK_DISTANCE, c.out("link", (F, cap), I32))
    return c


def link_ref(coords, counts, ms):
    counts = clean_counts(counts, coords.shape[1])
    return {"link": T.link_particles_movie(coords.astype(np.int32), counts, LINK_DISTANCE, ms)}


LINK_MS = np.array([0, 0, 1, 0], np.uint8)


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("ms", [None, LINK_MS], ids=["one_movie", "movie_start"])
@pytest.mark.parametrize("cap", [1, 7, 9, 65])
def test_link_frames_placement(cap, ms, mis):
    counts = [cap, (cap + 1) // 2, cap, 0]                               # 0 and cap; both sides play rows
    coords, counts, _ = scene(cap, 4, 20 + cap, counts)
    want = link_ref(coords, counts, ms)
    assert (want["link"][1] >= 0).any() and (ms is not None or (want["link"][2] >= 0).any())
    a = link_call(coords, counts, ms, mis)
    check_all(a, want)                                                    # every entry is written, -1 beyond the count
    same_results(a, link_call(zero_beyond(coords, counts), counts, ms, mis))


@pytest.mark.parametrize("cap", [1, 7, 9, 65])
def test_link_frames_hostile_counts(cap):
    coords, counts, _ = scene(cap, 4, 30 + cap, [cap, (cap + 1) // 2, cap, 0])
    raw = counts.copy()
    raw[0], raw[2], raw[3] = cap + 3, cap + 3, -2
    check_all(link_call(coords, G.bounded(raw, 0, cap, 8), None), link_ref(coords, raw, None))


def gaps_case(cap, F, seed):
    """a blinking scene with one frame in which nothing is detected, linked by the restatement"""
    coords, counts, who = scene(cap, F, seed, dark_frame=3)
    link = np.full((F, cap), GARBAGE32, np.int64)
    host = T.link_particles_movie(coords.astype(np.int32), counts.astype(np.int32), LINK_DISTANCE, None)
    for f in range(F):
        link[f, :counts[f]] = host[f, :counts[f]]
    return coords, counts, link


def gaps_call(coords, counts, link, ms, max_gap, mis=0, ws_fill=G.POISON):
    c = Call("mivit_close_gaps", mis)
    F, cap = coords.shape[:2]
    ws = c.work(F * cap, U8, ws_fill)
    c.run(c.inp("coords", coords, I32), c.inp("count", counts, I32), c.inp("link", link, I32),
          c.inp("movie_start", ms, U8) if ms is not None else None, F, cap, max_gap, LINK_DISTANCE,
          c.out("gap_partner", (F, cap), I32), c.out("gap_frames", (F, cap), I32), ws, ws.nbytes)
    return c


def gaps_ref(coords, counts, link, ms, max_gap):
    counts = clean_counts(counts, coords.shape[1])
    gp, gf = T._close_gaps_numpy(coords.astype(np.int32), counts, clean_links(link, counts), max_gap, LINK_DISTANCE, ms_bool(ms))
    return {"gap_partner": gp, "gap_frames": gf}


GAPS_MS = np.array([0, 0, 0, 0, 0, 1], np.uint8)


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("ms", [None, GAPS_MS], ids=["one_movie", "movie_start"])
@pytest.mark.parametrize("max_gap", [1, 3])
@pytest.mark.parametrize("cap", [7, 65])
def test_close_gaps_placement(cap, max_gap, ms, mis):
    coords, counts, link = gaps_case(cap, 6, 40 + cap)
    want = gaps_ref(coords, counts, link, ms, max_gap)
    assert (want["gap_frames"] == 2).any() and ((want["gap_frames"] > 2).any() or max_gap == 1)
    a = gaps_call(coords, counts, link, ms, max_gap, mis)
    check_all(a, want)                                                    # every entry is defined
    same_results(a, gaps_call(zero_beyond(coords, counts), counts, zero_beyond(link, counts), ms, max_gap, mis))


@pytest.mark.parametrize("cap", [7, 65])
def test_close_gaps_workspace_carries_no_state(cap):
    coords, counts, link = gaps_case(cap, 6, 50 + cap)
    big = gaps_call(*gaps_case(cap, 8, 60 + cap), None, 3)
    first = gaps_call(coords, counts, link, None, 3, ws_fill=0xFF)
    check_all(first, gaps_ref(coords, counts, link, None, 3))
    for fill in (0x00, big.ws.body_bytes()[:6 * cap]):
        same_results(first, gaps_call(coords, counts, link, None, 3, ws_fill=fill))


def unlinked_slots(link, counts, k):
    """k detections (f >= 1, j < count[f]) whose link is -1, from different frames where possible"""
    slots = [(f, int(j)) for f in range(1, len(link)) for j in np.flatnonzero(link[f, :counts[f]] == -1)[:2]]
    assert len(slots) >= k, "the scene has too few unlinked detections"
    return slots[:k]


@pytest.mark.parametrize("cap", [7, 65])
def test_close_gaps_hostile(cap):
    coords, counts, link = gaps_case(cap, 6, 70 + cap)
    assert counts[0] == cap and counts[3] == 0
    raw_counts, raw_link = counts.copy(), link.copy()
    raw_counts[0], raw_counts[3] = cap + 3, -2
    for (f, j), v in zip(unlinked_slots(link, counts, 3), (-5, None, cap + 3)):
        raw_link[f, j] = counts[f - 1] if v is None else v               # -5, count[f - 1], cap + 3: all count as -1
    raw_link[:, :][beyond(counts, cap)] = GARBAGE32
    inside = ~beyond(counts, cap)
    G.bounded(raw_link[inside], -1, cap - 1, 8)                          # a link indexes coords [., cap, 2] (8 B) and the byte flags
    c = gaps_call(coords, G.bounded(raw_counts, 0, cap, 8), raw_link, None, 3)
    check_all(c, gaps_ref(coords, raw_counts, raw_link, None, 3))
    check_all(c, gaps_ref(coords, counts, link, None, 3))                 # ... which is the result of the well-formed input


def chain_call(link, counts, ms, n_tracks, mis=0):
    c = Call("mivit_chain_tracks", mis)
    F, cap = link.shape
    c.run(c.inp("link", link, I32), c.inp("count", counts, I32), c.inp("movie_start", ms, U8) if ms is not None else None, F, cap,
          c.out("ids", (F, cap), I32), c.out("lengths", n_tracks, I32), c.out("n_tracks", 1, I32))
    return c


def chain_ref(link, counts, ms, gaps=None, max_gap=8):
    """-> (want, written); lengths in full ([F * cap], zeros beyond the last track)"""
    F, cap = link.shape
    counts = clean_counts(counts, cap)
    gp, gf = clean_gaps(gaps[0], gaps[1], counts, max_gap) if gaps else (None, None)
    ids, lengths, n = T._chain_numpy(clean_links(link, counts), counts, ms_bool(ms), gp, gf)
    return {"ids": ids, "lengths": lengths, "n_tracks": np.array([n])}, {"ids": ~beyond(counts, cap)}


CHAIN_MS = np.array([0, 0, 0, 1, 0], np.uint8)


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("ms", [None, CHAIN_MS], ids=["one_movie", "movie_start"])
@pytest.mark.parametrize("cap", [7, 257])
def test_chain_tracks_placement(cap, ms, mis):
    _, counts, who = scene(cap, 5, 80 + cap, dark_frame=None)
    link = links_of(who, cap, 1)[0]
    want, written = chain_ref(link, counts, ms)
    n = int(want["n_tracks"][0])
    assert cap < n < 5 * cap and want["lengths"][:n].max() == (5 if ms is None else 3)
    want["lengths"] = want["lengths"][:n]                                 # exactly n_tracks entries: the header says that suffices
    a = chain_call(link, counts, ms, n, mis)
    check_all(a, want, written)
    same_results(a, chain_call(zero_beyond(link, counts), counts, ms, n, mis), ["lengths", "n_tracks"])


@pytest.mark.parametrize("cap", [7, 257])
def test_chain_tracks_hostile(cap):
    _, counts, who = scene(cap, 5, 90 + cap, dark_frame=2)
    link = links_of(who, cap, 1)[0]
    raw_counts, raw_link = counts.copy(), link.copy()
    raw_counts[0], raw_counts[2] = cap + 3, -2
    for (f, j), v in zip(unlinked_slots(link, counts, 3), (-5, None, cap + 3)):
        raw_link[f, j] = counts[f - 1] if v is None else v
    G.bounded(raw_link[~beyond(counts, cap)], -1, cap - 1, 4)             # a link indexes the ids of the frame before (LDS, 4 B)
    want, written = chain_ref(raw_link, raw_counts, None)
    clean, _ = chain_ref(link, counts, None)
    n = int(want["n_tracks"][0])
    assert all(bits_equal(want[k], clean[k]) for k in want)
    want["lengths"] = want["lengths"][:n]
    check_all(chain_call(raw_link, G.bounded(raw_counts, 0, cap, 4), None, n), want, written)


def chain_gaps_call(link, gp, gf, counts, ms, max_gap, mis=0):
    c = Call("mivit_chain_tracks_gaps", mis)
    F, cap = link.shape
    c.run(c.inp("link", link, I32), c.inp("gap_partner", gp, I32), c.inp("gap_frames", gf, I32), c.inp("count", counts, I32),
          c.inp("movie_start", ms, U8) if ms is not None else None, F, cap, max_gap, c.out("ids", (F, cap), I32),
          c.out("lengths", F * cap, I32), c.out("n_tracks", 1, I32))
    return c


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("cap", [7, 257])
def test_chain_tracks_gaps_placement(cap, mis):
    _, counts, who = scene(cap, 12, 100 + cap, p_dark=0.5, dark_frame=5)  # F = 12, max_gap = 8: the ring of 10 frames wraps
    link, gp, gf = links_of(who, cap, 8)
    want, written = chain_ref(link, counts, None, (gp, gf))
    assert gf[~beyond(counts, cap)].max() >= 6 and (gf[~beyond(counts, cap)] == 2).any()
    plain, _ = chain_ref(link, counts, None)
    assert int(want["n_tracks"][0]) < int(plain["n_tracks"][0])
    a = chain_gaps_call(link, gp, gf, counts, None, 8, mis)
    check_all(a, want, written)                                           # lengths [F * cap]: "cleared here", every entry
    zeros = [zero_beyond(x, counts) for x in (link, gp, gf)]
    same_results(a, chain_gaps_call(*zeros, counts, None, 8, mis), ["lengths", "n_tracks"])


@pytest.mark.parametrize("cap", [7, 257])
def test_chain_tracks_gaps_hostile(cap):
    F, max_gap = 12, 8
    _, counts, who = scene(cap, F, 110 + cap, p_dark=0.5, dark_frame=5)
    link, gp, gf = links_of(who, cap, max_gap)
    raw_counts, raw_link, raw_gp, raw_gf = counts.copy(), link.copy(), gp.copy(), gf.copy()
    raw_counts[0], raw_counts[5] = cap + 3, -2
    inside = ~beyond(counts, cap)
    # every slot is a detection that continues a track across a gap: a hostile link leaves it so, a hostile gap entry makes it
    # the first detection of a new track
    gapped = [(f, int(j)) for f in range(F) for j in np.flatnonzero((gf[f] >= 2) & inside[f])[:2]]
    early = [(f, j) for f, j in gapped if f <= max_gap]
    rest = [s for s in gapped if s != early[0]]
    assert len(rest) >= 6
    for (f, j), v in zip(rest[:3], (-5, None, cap + 3)):
        raw_link[f, j] = counts[f - 1] if v is None else v
    (f, j), (f2, j2), (f3, j3), (f4, j4) = rest[3], rest[4], early[0], rest[5]
    raw_gf[f, j] = 1                                                      # g = 1: not a gap
    raw_gf[f2, j2] = max_gap + 2                                          # g beyond max_gap + 1
    raw_gf[f3, j3] = f3 + 1                                               # g > f: beyond frame 0
    raw_gp[f4, j4] = counts[f4 - gf[f4, j4]]                              # the partner frame has no such detection
    G.bounded(raw_link[inside], -1, cap - 1, 4), G.bounded(raw_gp[inside], -1, cap - 1, 4)
    G.bounded(raw_gf[inside], 0, max_gap + 1, cap * 4)                    # g selects a frame of ids in the LDS ring, cap * 4 B each
    want, written = chain_ref(raw_link, raw_counts, None, (raw_gp, raw_gf))
    clean, _ = chain_ref(link, counts, None, (gp, gf))
    assert int(want["n_tracks"][0]) == int(clean["n_tracks"][0]) + 4
    c = chain_gaps_call(raw_link, raw_gp, raw_gf, G.bounded(raw_counts, 0, cap, 4), None, max_gap)
    check_all(c, want, written)


# ----------------------------------------------------------------------------------------------------------------------
# mivit_dog_peaks
# ----------------------------------------------------------------------------------------------------------------------
DOG_SHAPE = (3, 19, 67)                                                   # 2 x 2 tiles of 16 x 64 with partial edge tiles
DOG_MIN_DISTANCE = 3


@functools.lru_cache(maxsize=None)
def dog_movie(seed=0, frames=3):
    """spots in all four tiles on a noisy background; frame 1 is flat -> (movie, dog, per frame (coords, n_candidates))"""
    rng = np.random.default_rng(seed)
    _, H, W = DOG_SHAPE
    yy, xx = np.mgrid[0:H, 0:W]
    mov = np.zeros((frames, H, W))
    for f in range(frames):
        for y, x in ((4, 10), (17, 30), (8, 65), (18, 66), (2, 50)):
            a = rng.uniform(80, 160)
            mov[f] += a * np.exp(-((yy - y - rng.uniform(-1, 1)) ** 2 + (xx - x - rng.uniform(-1, 1)) ** 2) / (2 * 1.2 ** 2))
    mov = (mov + 10.0 + rng.uniform(0, 1, mov.shape)).astype(np.float32)
    mov[1] = 7.0
    mov.setflags(write=False)
    return mov


def dog_weights():
    return T.gaussian_half_kernel(1.0), T.gaussian_half_kernel(2.0)      # radii 4 and 8


def dog_call(movie, cap, thr, store_dog, mis=0, ws_fill=G.POISON, out_fill=None):
    c = Call("mivit_dog_peaks", mis)
    F, H, W = movie.shape
    w1, w2 = dog_weights()
    wsb = N.lib.mivit_dog_peaks_workspace_bytes(F, H, W, cap, 1 if store_dog else 0)
    ws = c.work(wsb, U8, ws_fill)
    c.run(c.inp("movie", movie, F32), F, H, W, w1.ctypes.data, len(w1) - 1, w2.ctypes.data, len(w2) - 1, thr, DOG_MIN_DISTANCE,
          cap, c.out("count", F, I32, out_fill), c.out("n_candidates", F, I32, out_fill), c.out("coords", (F, cap, 2), I32, out_fill),
          c.out("values", (F, cap), F32, out_fill), c.out("dog", (F, H, W), F32, out_fill) if store_dog else None, ws, wsb)
    return c


def dog_ref(movie, cap, thr, store_dog):
    F = len(movie)
    dog = T._dog_numpy(movie, *dog_weights())
    want = {"count": np.zeros(F, np.int32), "n_candidates": np.zeros(F, np.int32), "coords": np.zeros((F, cap, 2), np.int32),
            "values": np.zeros((F, cap), np.float32)}
    for f in range(F):
        yx, want["n_candidates"][f] = T._peaks_numpy(dog[f], thr, DOG_MIN_DISTANCE)
        n = min(len(yx), cap)
        want["count"][f] = n
        want["coords"][f, :n], want["values"][f, :n] = yx[:n], dog[f][yx[:n, 0], yx[:n, 1]]
    kept = ~beyond(want["count"], cap)
    if store_dog:
        want["dog"] = dog
    return want, {"coords": kept[:, :, None], "values": kept}


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("store_dog", [1, 0], ids=["dog returned", "dog in the workspace"])
def test_dog_peaks_placement(store_dog, mis):
    movie = dog_movie()
    want, written = dog_ref(movie, 8, 0.2, store_dog)
    assert want["count"].tolist()[1] == 0 and min(want["count"][0], want["count"][2]) >= 3 and want["n_candidates"].max() <= 8
    a = dog_call(movie, 8, 0.2, store_dog, mis)
    check_all(a, want, written)
    b = dog_call(movie, 8, 0.2, store_dog, mis, out_fill="zero")          # what an output held before is not read
    for name in want:
        w = np.broadcast_to(written.get(name, True), a.outs[name].shape)
        assert bits_equal(a.outs[name].numpy()[w], b.outs[name].numpy()[w]), name
        assert (b.outs[name].numpy()[~w] == 0).all(), name


@pytest.mark.parametrize("store_dog", [1, 0], ids=["dog returned", "dog in the workspace"])
def test_dog_peaks_overflow_stays_inside(store_dog):
    """more candidates than cap: reported in n_candidates; the frame's peaks are then incomplete (which candidates were stored
    is up to the atomics), but coords, values and the candidate keys stay inside their buffers"""
    movie = dog_movie()
    want, _ = dog_ref(movie, 2, 0.001, store_dog)
    assert want["n_candidates"][0] > 2 and want["n_candidates"][2] > 2
    c = dog_call(movie, 2, 0.001, store_dog)
    expect(c, "n_candidates", want["n_candidates"])
    count = c.outs["count"].numpy()
    assert count[1] == 0 and (1 <= count[[0, 2]]).all() and (count <= 2).all()
    kept = ~beyond(count, 2)
    assert c.outs["coords"].untouched(~np.broadcast_to(kept[:, :, None], (3, 2, 2))) and c.outs["values"].untouched(~kept)
    if store_dog:
        expect(c, "dog", T._dog_numpy(movie, *dog_weights()))


@pytest.mark.parametrize("store_dog", [1, 0], ids=["dog returned", "dog in the workspace"])
def test_dog_peaks_workspace_carries_no_state(store_dog):
    movie = dog_movie()
    big = dog_call(dog_movie(1, 4), 8, 0.001, store_dog)                  # more frames, a low threshold: keys in every slot
    first = dog_call(movie, 8, 0.2, store_dog, ws_fill=0xFF)
    for fill in (0x00, big.ws.body_bytes()[:first.ws.nbytes]):
        other = dog_call(movie, 8, 0.2, store_dog, ws_fill=fill)
        kept = ~beyond(first.outs["count"].numpy(), 8)
        for name in first.outs:
            w = {"coords": kept[:, :, None], "values": kept}.get(name, True)
            w = np.broadcast_to(w, first.outs[name].shape)
            assert bits_equal(first.outs[name].numpy()[w], other.outs[name].numpy()[w]), name


# ----------------------------------------------------------------------------------------------------------------------
# mivit_refine_gaussian, mivit_fit_spots_mle: no indices, so placement and the misaligned case only
# ----------------------------------------------------------------------------------------------------------------------
FIT_SIZES = (1, 65, 513, 64 * 256 + 1)                                    # 1 lane a workgroup, 1, 2, full waves with a one-patch tail
FIT_SET = 65


def fit_close(got, want, what):
    """tracking_common.KERNEL_FIT_RTOL relative, as tests/test_localize_gpu.py measures it; NaN where the restatement has NaN"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want == got, 0.0, np.abs(got - want) / np.abs(want))
    worst = float(np.nanmax(rel)) if rel.size else 0.0
    print(f"{what}: worst relative difference {worst:.3e}")
    assert worst <= tc.KERNEL_FIT_RTOL, (what, worst)


@functools.lru_cache(maxsize=None)
def refine_set(P):
    patches = tc.spot_patches(FIT_SET, P)
    return patches, T._refine_numpy(patches, T.FIT_XTOL)


@functools.lru_cache(maxsize=None)
def mle_set(name, fit_sigma):
    patches = LC.case_patches(name, FIT_SET)
    kw = dict(LC.camera_kwargs(name), fit_sigma=fit_sigma)
    return patches, kw, T._fit_mle_numpy(patches, xtol=T.FIT_XTOL, **kw)


def refine_check(P, n, mis):
    patches, ref = refine_set(P)
    c = Call("mivit_refine_gaussian", mis)
    c.run(c.inp("patches", LC.tiled(patches, n), F32), n, P, T.FIT_XTOL, c.out("params", (n, 5), F64), c.out("peak", n, F32),
          c.out("status", n, I32))
    want = dict(zip(("params", "peak", "status"), (LC.tiled(a, n) for a in ref)))
    check_all(c, want, close={"params": fit_close})


def mle_check(name, fit_sigma, n, mis):
    patches, kw, ref = mle_set(name, fit_sigma)
    P = patches.shape[1]
    c = Call("mivit_fit_spots_mle", mis)
    c.run(c.inp("patches", LC.tiled(patches, n), F32), n, P, kw["gain"], kw["offset"], kw["read_var"], kw["sigma0"],
          1 if fit_sigma else 0, T.FIT_XTOL, c.out("params", (n, 5), F64), c.out("crlb", (n, 5), F64), c.out("deviance", n, F64),
          c.out("status", n, I32), c.out("iterations", n, I32))
    want = dict(zip(("params", "crlb", "deviance", "status", "iterations"), (LC.tiled(a, n) for a in ref)))
    check_all(c, want, close={"params": fit_close, "crlb": fit_close, "deviance": fit_close})
    if not fit_sigma:
        assert (c.outs["params"].numpy()[:, 3] == kw["sigma0"]).all() and (c.outs["crlb"].numpy()[:, 3] == 0.0).all()


@pytest.mark.parametrize("n,mis", [(n, 0) for n in FIT_SIZES] + [(65, 1)])
@pytest.mark.parametrize("P", [3, 15])
def test_refine_gaussian_placement(P, n, mis):
    refine_check(P, n, mis)


@pytest.mark.parametrize("n,mis", [(n, 0) for n in FIT_SIZES] + [(65, 1)])
@pytest.mark.parametrize("name,fit_sigma", [("p3_fixed", False), ("p15_camera", True), ("p15_camera", False)])
def test_fit_spots_mle_placement(name, fit_sigma, n, mis):
    mle_check(name, fit_sigma, n, mis)


# ----------------------------------------------------------------------------------------------------------------------
# mivit_trajectory_features
# ----------------------------------------------------------------------------------------------------------------------
FEAT_T = 40


def feat_walks(n, dtype, seed=23):
    rng = np.random.default_rng(seed)
    sc_ = 10 ** rng.uniform(-1.0, 0.3, (n, 1, 1))
    return (np.cumsum(rng.standard_normal((n, FEAT_T, 2)) * sc_ + 0.3 * sc_, axis=1) + rng.standard_normal((n, 1, 2)) * 20).astype(dtype)


def feat_call(traj, npos, with_avg, mis=0, ws_fill=G.POISON):
    c = Call("mivit_trajectory_features", mis)
    n, steps, _ = traj.shape
    tdt, code = (F32, N.F32) if traj.dtype == np.float32 else (F64, N.F64)
    wsb = N.lib.mivit_trajectory_features_workspace_bytes(n, steps, npos)
    ws = c.work(wsb, F64, ws_fill)
    c.run(c.inp("traj", traj, tdt), code, n, steps, npos, 1.0, c.out("feats", (n, 25), F64),
          c.out("avg", (n, steps // npos, 2), tdt) if with_avg else None, ws, wsb)
    return c


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("with_avg", [1, 0], ids=["avg", "avg NULL"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("npos", [1, 3])
@pytest.mark.parametrize("n", [1, 65])
def test_trajectory_features_placement(n, npos, dtype, with_avg, mis):
    traj = feat_walks(n, dtype)
    nf, rest = FEAT_T // npos, FEAT_T % npos
    ref, ref_avg = tf.host_features(traj, npos=npos, dt=1.0, with_average=True)
    garbage = traj.copy()
    if rest:                                                              # the trailing sub-steps are ignored: poison them
        garbage[:, FEAT_T - rest:] = np.frombuffer(b"\xff" * 8, dtype)[0]
    a = feat_call(garbage, npos, with_avg, mis)
    assert not a.outs["feats"].unchanged().numpy().any() and not G.is_poison(a.outs["feats"].numpy()).any()
    got = a.outs["feats"].numpy()
    msgs = tf.check_against(got, ref, np.array([max(tf.max_sq(p), 1e-300) for p in ref_avg.astype(np.float64)]), [nf] * n)
    assert not msgs, msgs
    if with_avg:
        expect(a, "avg", ref_avg)                                         # averaged in the input precision: bitwise
    if rest:
        zeroed = traj.copy()
        zeroed[:, FEAT_T - rest:] = 0
        same_results(a, feat_call(zeroed, npos, with_avg, mis))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("npos", [1, 3])
def test_trajectory_features_workspace_carries_no_state(npos, dtype):
    traj = feat_walks(65, dtype)
    big = feat_call(feat_walks(130, dtype, seed=24), 1, 1)                # a larger problem: 130 walks of 40 frames
    first = feat_call(traj, npos, 1, ws_fill=0xFF)
    for fill in (0x00, big.ws.body_bytes()[:first.ws.nbytes].view(F64)):
        same_results(first, feat_call(traj, npos, 1, ws_fill=fill))
