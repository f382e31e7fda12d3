"""GPU: the kernels of csrc/hmm.hip (ops.hmm_estep, ops.hmm_viterbi) against the numpy restatements of helpers/msd.py, which
tests/test_hmm.py holds against two oracles on the same common set, and the paths that reach them: helpers/msd.
fit_diffusion_states and tracking.estimate_track_diffusion(states=...).

The E-step is compared within hmm_common.HMM_TOL (derived there: exp and log are the only operations that may differ) and its
state on EVERY row (tests/test_hmm.py holds the gap of the two largest gamma above 1e-6 on every row of the common set).  The
Viterbi kernel has no transcendental function -- the logarithms are its inputs and both sides get the same ones -- and is
compared bit for bit."""
import numpy as np
import pytest
import torch

import hmm_common as hc
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as msd_mod
from moleculardiffusion_mivit_amd.helpers import tracking as trk

pytestmark = pytest.mark.gpu

SETS = list(hc.parameter_sets())
NAMES = ("gamma", "state", "xi", "g_sum", "gq_sum", "g_first", "loglik")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                 # a copy: the common inputs are read-only


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def _estep(pos, offsets, v, A, pi):
    out = ops.hmm_estep(_dev(pos), _dev(np.asarray(offsets).astype(np.int32)), _dev(v), _dev(A), _dev(pi))
    torch.cuda.synchronize()
    assert out[0].shape == (len(pos), len(v)) and out[1].dtype == torch.int32 and out[2].shape == (len(offsets) - 1, len(v), len(v))
    return dict(zip(NAMES, (o.cpu().numpy() for o in out)))


def _viterbi(pos, offsets, v, A, pi):
    """-> (state, logp of the kernel, the logarithms it was given: torch.log on the device, as ops.hmm_viterbi takes them)"""
    dv, dA, dpi = _dev(v), _dev(A), _dev(pi)
    state, logp = ops.hmm_viterbi(_dev(pos), _dev(np.asarray(offsets).astype(np.int32)), dv, dA, dpi)
    torch.cuda.synchronize()
    assert state.dtype == torch.int32 and state.shape == (len(pos),) and logp.shape == (len(offsets) - 1,)
    return state.cpu().numpy(), logp.cpu().numpy(), tuple(torch.log(t).cpu().numpy() for t in (dv, dA, dpi))


def _same_nan(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want))


def _check_estep(got, want, what):
    assert _same_nan(got["gamma"], want["gamma"]), what
    ok = ~np.isnan(want["gamma"])
    assert np.all(np.abs(got["gamma"][ok] - want["gamma"][ok]) <= hc.HMM_TOL), (what, float(np.abs(got["gamma"][ok] - want["gamma"][ok]).max()))
    assert np.array_equal(got["state"], want["state"]), what
    for s in NAMES[2:]:
        assert _same_nan(got[s], want[s]) and np.array_equal(np.isinf(got[s]), np.isinf(want[s])), (what, s)
        fin = np.isfinite(want[s])
        hc.close(got[s][fin], want[s][fin], (what, s))


@pytest.mark.parametrize("name", SETS)
def test_estep_equals_the_restatement_on_every_track(name):
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()[name]
    want = dict(zip(NAMES, msd_mod._hmm_estep_numpy(pos, offsets, v, A, pi)))
    got = _estep(pos, offsets, v, A, pi)
    _check_estep(got, want, name)
    lengths = np.diff(offsets)
    assert (got["state"][offsets[:-1][lengths == 1]] == -1).all() and np.isnan(got["loglik"][lengths < 2]).all()
    assert np.isfinite(got["loglik"][lengths >= 2]).all()


@pytest.mark.parametrize("name", SETS)
def test_viterbi_is_bitwise_the_restatement(name):
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()[name]
    state, logp, (logv, logA, logpi) = _viterbi(pos, offsets, v, A, pi)
    want_state, want_logp = msd_mod._hmm_viterbi_numpy(pos, offsets, v, logv, logA, logpi)
    assert np.array_equal(state, want_state)
    assert _same_nan(logp, want_logp) and np.array_equal(_bits(logp)[~np.isnan(logp)], _bits(want_logp)[~np.isnan(logp)])


def _slice(out, offsets, k):
    a, b = offsets[k], offsets[k + 1]
    return [_bits(out[s][a:b]) for s in ("gamma", "state")] + [_bits(out[s][k]) for s in NAMES[2:]]


def test_a_track_is_bitwise_the_same_alone_and_anywhere_in_a_batch():
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()["K3"]
    lengths = np.diff(offsets)
    picks = [int(np.argmax(lengths)), int(np.nonzero(lengths == 9)[0][0]), len(lengths) - 3]      # 513 rows, 9 rows, planted
    tracks = [pos[a:b] for a, b in zip(offsets[:-1], offsets[1:])]
    others = [t for i, t in enumerate(tracks) if i not in picks]

    def run(batch):
        p, off = np.concatenate(batch), np.concatenate([[0], np.cumsum([len(t) for t in batch])])
        e = _estep(p, off, v, A, pi)
        s, lp, _ = _viterbi(p, off, v, A, pi)
        return e, s, lp, off

    for k in picks:
        e, s, lp, off = run([tracks[k]])
        alone = _slice(e, off, 0) + [s, _bits(lp[0])]
        cases = [[tracks[k]], [tracks[k]] + others, others + [tracks[k]]]
        for n in (1, 7, 8, 9, 17):
            cases.append((others[:n // 2] + [tracks[k]] + others[n // 2:n - 1]))
            assert len(cases[-1]) == n
        for batch in cases:
            at = next(i for i, t in enumerate(batch) if t is tracks[k])
            e, s, lp, off = run(batch)
            got = _slice(e, off, at) + [s[off[at]:off[at + 1]], _bits(lp[at])]
            assert all(np.array_equal(g, w) for g, w in zip(got, alone)), (k, len(batch), at)


def test_a_nan_row_poisons_its_own_track_only():
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()["K2"]
    base = _estep(pos, offsets, v, A, pi)
    bs, blp, _ = _viterbi(pos, offsets, v, A, pi)
    j = int(np.argmax(np.diff(offsets)))
    bad = np.array(pos)
    bad[offsets[j] + 100, 1] = np.nan
    got = _estep(bad, offsets, v, A, pi)
    gs, glp, _ = _viterbi(bad, offsets, v, A, pi)
    a, b = offsets[j], offsets[j + 1]
    assert np.isnan(got["gamma"][a:b]).all() and (got["state"][a:b] == -1).all() and np.isnan(got["loglik"][j])
    assert all(np.isnan(got[s][j]).all() for s in NAMES[2:]) and np.isnan(glp[j])
    keep = np.ones(len(pos), bool)
    keep[a:b] = False
    for s in ("gamma", "state"):
        assert np.array_equal(_bits(got[s][keep]), _bits(base[s][keep])), s
    for s in NAMES[2:]:
        assert np.array_equal(_bits(np.delete(got[s], j, axis=0)), _bits(np.delete(base[s], j, axis=0))), s
    assert np.array_equal(gs[keep], bs[keep]) and np.array_equal(_bits(np.delete(glp, j)), _bits(np.delete(blp, j)))


def test_underflow_gives_minus_infinity_on_its_own_track_only():
    pos, offsets = hc.common_tracks()
    v, A, _ = hc.parameter_sets()["K2_identity"]
    pi = np.array([1.0, 0.0])                                              # the narrow state only: the large step is impossible
    want = dict(zip(NAMES, msd_mod._hmm_estep_numpy(pos, offsets, v, A, pi)))
    assert (want["loglik"] == -np.inf).sum() == 1
    _check_estep(_estep(pos, offsets, v, A, pi), want, "underflow")


def test_no_length_limit():
    """one track of 5 000 rows, past ops.SEG_MAX_LEN: the recurrence's state lives in global memory"""
    assert 5000 > ops.SEG_MAX_LEN
    pos, s = hc.switching_track(np.random.default_rng(3), 5000, hc.DS3, hc.M3)
    offsets = np.array([0, 5000])
    v, A, pi = hc.parameter_sets()["K3"]
    want = dict(zip(NAMES, msd_mod._hmm_estep_numpy(pos, offsets, v, A, pi)))
    got = _estep(pos, offsets, v, A, pi)
    g = np.sort(want["gamma"], axis=1)
    sure = g[:, -1] - g[:, -2] >= hc.MIN_GAP                               # a random track: leave the rows without a margin out of state
    assert sure.mean() >= 0.999
    got["state"], want["state"] = got["state"][sure], want["state"][sure]
    _check_estep(got, want, "5000 rows")
    state, logp, (logv, logA, logpi) = _viterbi(pos, offsets, v, A, pi)
    want_state, want_logp = msd_mod._hmm_viterbi_numpy(pos, offsets, v, logv, logA, logpi)
    assert np.array_equal(state, want_state) and np.array_equal(_bits(logp), _bits(want_logp))
    assert float((state[:-1] == s).mean()) >= 0.9


def test_fit_on_the_gpu_equals_the_fit_on_the_cpu():
    """The two fits share the start (order statistics: exact on both sides) and differ in the E-step by exp and log (1e-14
    on the statistics, hmm_common) and in the M-step by the order in which torch sums the tracks' statistics on either
    device (1e-16 relative per sum).  EM maps a perturbation of its parameters into one of the same order per iteration (its
    rate is below 1 near the fixed point, above it in the first iterations by at most the condition of the start), so over
    the about 10 to 30 iterations of this fit the 1e-14 floor grows to 1e-12 at most; 1e-8 relative leaves four orders, and
    the same orders separate it from the convergence test's tol = 1e-8 * |loglik| deciding differently: n_iter is equal."""
    pos, offsets, truth = hc.planted_set(40)
    cpu = msd_mod.fit_diffusion_states(torch.from_numpy(np.array(pos)), torch.from_numpy(np.array(offsets)), 2)
    dev = msd_mod.fit_diffusion_states(_dev(pos), _dev(offsets), 2)
    assert all(dev[k].is_cuda for k in ("Ds", "M", "p0", "gamma", "state", "state_posterior", "occupancy"))
    print("cpu", cpu["Ds"], cpu["M"], cpu["n_iter"], cpu["loglik"], "gpu", dev["Ds"], dev["M"], dev["n_iter"], dev["loglik"])
    assert dev["n_iter"] == cpu["n_iter"] and dev["converged"] and cpu["converged"]
    assert dev["n_tracks_used"] == cpu["n_tracks_used"] == 40 and dev["n_increments"] == cpu["n_increments"]
    for k in ("Ds", "M", "p0"):
        assert torch.allclose(dev[k].cpu(), cpu[k], rtol=1e-8, atol=0), k
    assert abs(dev["loglik"] - cpu["loglik"]) <= 1e-8 * abs(cpu["loglik"]) and abs(dev["bic"] - cpu["bic"]) <= 1e-8 * abs(cpu["bic"])
    g = torch.sort(cpu["gamma"], dim=1)[0]
    sure = (g[:, 1] - g[:, 0] > 1e-6)
    assert float(sure.double().mean()) >= 0.99                             # the CPU side: the input leaves few rows undecided
    assert torch.equal(dev["state"].cpu()[sure], cpu["state"][sure])
    assert torch.equal(dev["state_posterior"].cpu()[sure], cpu["state_posterior"][sure])
    assert float((dev["state"].cpu().numpy()[truth >= 0] == truth[truth >= 0]).mean()) >= 0.9


def test_rejected_input():
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()["K2"]
    p, o, dv, dA, dpi = _dev(pos), _dev(offsets.astype(np.int32)), _dev(v), _dev(A), _dev(pi)
    v9 = torch.full((9,), 1.0, dtype=torch.float64, device="cuda")
    bad = [(p.float(), o, dv, dA, dpi), (p.cpu(), o, dv, dA, dpi), (p, o.long(), dv, dA, dpi), (p, o, dv.float(), dA, dpi),
           (p, o, dv, dA.cpu(), dpi), (p.reshape(-1), o, dv, dA, dpi), (torch.cat([p, p], dim=1), o, dv, dA, dpi),
           (p.repeat(1, 2)[:, ::2], o, dv, dA, dpi), (p, o, dv, dA.t(), dpi), (p, o, dv, dA[:, :1].contiguous(), dpi),
           (p, o, dv, torch.eye(3, dtype=torch.float64, device="cuda"), dpi), (p, o, dv, dA, dpi[:1].contiguous()),
           (p, o, v9, torch.eye(9, dtype=torch.float64, device="cuda"), v9 / 9), (p, o[:-1].contiguous(), dv, dA, dpi),
           (p, o.flip(0).contiguous(), dv, dA, dpi), (p, o[:0], dv, dA, dpi)]
    for f in (ops.hmm_estep, ops.hmm_viterbi):
        for args in bad:
            with pytest.raises(ValueError):
                f(*args)
    from moleculardiffusion_mivit_amd import _native as N
    assert N.lib.mivit_hmm_estep(None, 4, None, 1, 2, *([None] * 12)) != 0 and "null" in N.last_error()
    assert N.lib.mivit_hmm_estep(None, 4, None, 1, 9, *([None] * 12)) != 0 and "states" in N.last_error()
    assert N.lib.mivit_hmm_viterbi(None, -1, None, 1, 2, *([None] * 8)) != 0 and "negative" in N.last_error()
    assert N.lib.mivit_hmm_viterbi(None, 4, None, 1, 0, *([None] * 8)) != 0 and "states" in N.last_error()
    assert N.lib.mivit_hmm_estep(None, 0, None, 0, 2, *([None] * 12)) == 0                # no tracks: a no-op
    e = ops.hmm_estep(p[:0], o[:1], dv, dA, dpi)
    assert e[0].shape == (0, 2) and e[6].shape == (0,)


class MeanPixel(torch.nn.Module):
    def forward(self, seq):
        return seq.mean(dim=(1, 2, 3)).unsqueeze(1)


def _same(a, b):
    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


def test_end_to_end_on_a_movie_with_a_planted_change():
    """The movie of tests/test_segment_gpu.py, rebuilt here: 6 particles, 80 frames of 64 x 64, noise-free, Ds = (0.02, 1.0),
    every particle 40 frames in one state and 40 in the other.  A matched track is one that score_tracking gives to one
    particle with purity 1 and that has at least 2 * 4 + 5 rows on either side of frame 40."""
    Np, F_ = 6, 80
    path = torch.zeros(Np, F_, dtype=torch.int64)
    path[0::2, 40:] = 1
    path[1::2, :40] = 1
    props = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
    g = torch.Generator(device="cuda").manual_seed(11)
    movie, truth = gen.simulate_movie(Np, F_, 64, 64, None, 2, image_props=props, generator=g, device="cuda",
                                      states={"Ds": (0.02, 1.0), "M": np.eye(2), "path": path})
    model = MeanPixel().cuda()
    base = trk.estimate_track_diffusion(movie, model, 10, max_gap=2)
    res = trk.estimate_track_diffusion(movie, model, 10, max_gap=2, states={"K": 2})
    assert set(res) == set(base) | {"states"}
    for k in base:                                                         # the per-track entries, bit for bit
        assert _same(base[k], res[k]), k
    both = trk.estimate_track_diffusion(movie, model, 10, max_gap=2, states={"K": 2}, segment={})
    seg = trk.estimate_track_diffusion(movie, model, 10, max_gap=2, segment={})["segments"]
    assert set(both) == set(base) | {"states", "segments"} and all(_same(seg[k], both["segments"][k]) for k in seg)
    st = res["states"]
    print("Ds", st["Ds"], "M", st["M"], "n_iter", st["n_iter"])
    assert float(st["Ds"][0]) < 0.1 and float(st["Ds"][1]) > 0.25
    table, _ = trk.track_particles_tensors(movie, return_dog=False, max_gap=2)
    fr, y, x, tid, offsets = trk.tracks_table_by_track(table)[:5]
    score = trk.score_tracking(fr, y, x, tid, truth)
    assert torch.equal(score["track_id"], res["track_id"])
    n_rows, n_tracks = len(fr), len(res["track_id"])
    # run_offsets is a CSR over the same rows that refines offsets
    ro, rt, rs = st["run_offsets"], st["run_track"], st["run_state"]
    assert int(ro[0]) == 0 and int(ro[-1]) == n_rows and bool((ro[1:] > ro[:-1]).all())
    assert bool(torch.isin(offsets[:-1][offsets[1:] > offsets[:-1]], ro).all())
    assert torch.equal(rt, torch.searchsorted(offsets.contiguous(), ro[:-1], right=True) - 1)
    assert torch.equal(rs, st["state"][ro[:-1]]) and st["state"].shape == (n_rows,) and st["gamma"].shape == (n_rows, 2)
    run_of_row = torch.repeat_interleave(torch.arange(len(rt), device="cuda"), ro[1:] - ro[:-1])
    assert torch.equal(st["state"], rs[run_of_row])                        # constant on a run ...
    same_track = rt[1:] == rt[:-1]
    assert bool((rs[1:][same_track] != rs[:-1][same_track]).all())         # ... and maximal
    assert torch.equal(st["n_sequences"], (ro[1:] - ro[:-1]) // 10)
    assert bool((torch.isnan(st["D_model"]) == (st["n_sequences"] == 0)).all()) and st["D_model"].shape == rt.shape
    fr, offsets, state = fr.cpu().numpy(), offsets.cpu().numpy(), st["state"].cpu().numpy()
    need, checked = 2 * 4 + 5, 0
    for k in range(n_tracks):
        f = fr[offsets[k]:offsets[k + 1]]
        if int(score["particle_id"][k]) < 0 or float(score["purity"][k]) < 1.0 or f[0] > 40 - need or f[-1] < 40 + need:
            continue
        s = state[offsets[k]:offsets[k + 1]]
        change = np.nonzero(s[1:] != s[:-1])[0] + 1
        print(f"track {k}: frames {f[0]} .. {f[-1]}, the state changes at frames {f[change]}")
        assert len(change) == 1 and abs(int(f[change[0]]) - 40) <= 5, (k, f[change])
        checked += 1
    assert checked >= 1
