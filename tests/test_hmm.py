"""CPU: the numpy restatements of csrc/hmm.hip (helpers/msd._hmm_estep_numpy, _hmm_viterbi_numpy) against the two oracles of
tests/hmm_common.py, the margins that let tests/test_hmm_gpu.py compare states on every row, and the front ends
fit_diffusion_states / hmm_posteriors on arrays.  The tolerances are derived in hmm_common."""
import math

import numpy as np
import pytest
import torch

import hmm_common as hc
from moleculardiffusion_mivit_amd.helpers import msd as msd_mod
from moleculardiffusion_mivit_amd.helpers import tracking as trk

SETS = list(hc.parameter_sets())
STATS = ("xi", "g_sum", "gq_sum", "g_first")
_cache = {}


def restated(name):
    """The restatements on the common set under one parameter set, computed once -> dict."""
    if name not in _cache:
        pos, offsets = hc.common_tracks()
        v, A, pi = hc.parameter_sets()[name]
        gamma, state, xi, g_sum, gq_sum, g_first, loglik = msd_mod._hmm_estep_numpy(pos, offsets, v, A, pi)
        with np.errstate(divide="ignore"):
            path, logp = msd_mod._hmm_viterbi_numpy(pos, offsets, v, np.log(v), np.log(A), np.log(pi))
        _cache[name] = {"gamma": gamma, "state": state, "xi": xi, "g_sum": g_sum, "gq_sum": gq_sum, "g_first": g_first,
                        "loglik": loglik, "path": path, "logp": logp}
    return _cache[name]


def _compare(r, k, a, b, want, what):
    T = b - a - 1
    assert np.all(np.abs(r["gamma"][a:a + T] - want["gamma"]) <= hc.HMM_TOL), what
    assert np.array_equal(r["gamma"][b - 1], r["gamma"][b - 2]) and r["state"][b - 1] == r["state"][b - 2], what
    for s in STATS:
        hc.close(r[s][k], want[s], (what, s))
    hc.close(r["loglik"][k], want["loglik"], (what, "loglik"))
    hc.close(r["logp"][k] - T * hc.LOG_2PI, want["logp"], (what, "logp"))
    assert np.array_equal(r["path"][a:a + T], want["path"]) and r["path"][b - 1] == r["path"][b - 2], what
    assert np.array_equal(r["state"][a:a + T], np.argmax(want["gamma"], axis=1)), what


@pytest.mark.parametrize("name", [n for n in SETS if n != "K8"])
def test_restatements_equal_the_definition_on_short_tracks(name):
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()[name]
    r, checked = restated(name), 0
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        if not 1 <= b - a - 1 <= 10:
            continue
        want = hc.oracle_enumerate(pos[a:b], v, A, pi)
        assert want["gap"] >= hc.MIN_GAP, (name, k, want["gap"])
        _compare(r, k, a, b, want, (name, k))
        checked += 1
    assert checked >= 7


@pytest.mark.parametrize("name", SETS)
def test_restatements_equal_the_log_domain_oracle_on_every_track(name):
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()[name]
    r = restated(name)
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        if b - a < 2:
            assert np.isnan(r["loglik"][k]) and np.isnan(r["logp"][k]) and all(np.isnan(r[s][k]).all() for s in STATS)
            if b - a == 1:
                assert np.isnan(r["gamma"][a]).all() and r["state"][a] == -1 and r["path"][a] == -1
            continue
        assert np.isfinite(r["loglik"][k]), (name, k)                     # the track with the large step included
        _compare(r, k, a, b, hc.oracle_logdomain(pos[a:b], v, A, pi), (name, k))


@pytest.mark.parametrize("name", SETS)
def test_margins_of_the_common_set(name):
    """the two largest gamma of every row differ by at least MIN_GAP: what the GPU test's exact comparison of state rests on"""
    g = restated(name)["gamma"]
    g = g[~np.isnan(g).any(axis=1)]
    if g.shape[1] > 1:
        top = np.sort(g, axis=1)
        assert float((top[:, -1] - top[:, -2]).min()) >= hc.MIN_GAP
    assert np.all(np.abs(g.sum(axis=1) - 1.0) <= 1e-12)


def test_large_step_underflows_the_narrow_states_to_exact_zero():
    pos, offsets = hc.common_tracks()
    k = next(i for i in range(len(offsets) - 1) if hc.increments(pos[offsets[i]:offsets[i + 1]]).max(initial=0) > 1e4)
    g = restated("K3")["gamma"][offsets[k]:offsets[k + 1]]
    row = int(np.argmax(hc.increments(pos[offsets[k]:offsets[k + 1]])))
    assert g[row, 0] == 0.0 and g[row, 1] == 0.0 and g[row, 2] == 1.0 and np.isfinite(restated("K3")["loglik"][k])


def test_underflow_and_nan_end_one_track_only():
    pos, offsets = hc.common_tracks()
    v, A, pi = hc.parameter_sets()["K2_identity"]
    base = msd_mod._hmm_estep_numpy(pos, offsets, v, A, np.array([1.0, 0.0]))            # the narrow state only: the large step is impossible
    k = next(i for i in range(len(offsets) - 1) if hc.increments(pos[offsets[i]:offsets[i + 1]]).max(initial=0) > 1e4)
    assert base[6][k] == -np.inf and np.isnan(base[0][offsets[k]:offsets[k + 1]]).all()
    assert (base[1][offsets[k]:offsets[k + 1]] == -1).all() and np.isnan(base[2][k]).all()
    assert np.isfinite(np.delete(base[6], k)[np.diff(offsets)[np.arange(len(offsets) - 1) != k] > 1]).all()
    bad = np.array(pos)
    j = int(np.argmax(np.diff(offsets)))                                   # the 513-row track
    bad[offsets[j] + 100, 1] = np.nan
    v, A, pi = hc.parameter_sets()["K2"]
    got = msd_mod._hmm_estep_numpy(bad, offsets, v, A, pi)
    want = restated("K2")
    assert np.isnan(got[6][j]) and np.isnan(got[0][offsets[j]:offsets[j + 1]]).all()
    keep = np.ones(len(pos), bool)
    keep[offsets[j]:offsets[j + 1]] = False
    assert np.array_equal(got[0][keep], want["gamma"][keep], equal_nan=True) and np.array_equal(got[1][keep], want["state"][keep])
    assert np.array_equal(np.delete(got[6], j), np.delete(want["loglik"], j), equal_nan=True)


@pytest.fixture(scope="module")
def fit200():
    pos, offsets, truth = hc.planted_set(200)
    return msd_mod.fit_diffusion_states(pos, offsets, 2), truth


def test_fit_recovers_the_planted_states(fit200):
    """200 tracks of 20 to 120 rows under Ds = (0.05, 1.0), M = ((0.95, 0.05), (0.1, 0.9)): about 4 500 of the 13 700
    increments are in the rarer state, so D has a standard error of 1 / sqrt(4 500) = 1.5 % and a transition probability p
    one of sqrt(p (1 - p) / 4 500) = 0.0045 at p = 0.1; the thresholds are six standard errors (10 %, 0.03).  A row is
    misclassified where its neighbourhood does not tell the states apart: the prototype measured 0.978, the bound is 0.95."""
    fit, truth = fit200
    print("Ds", fit["Ds"], "M", fit["M"], "p0", fit["p0"], "n_iter", fit["n_iter"], "loglik", fit["loglik"])
    assert fit["converged"] and fit["n_tracks_used"] == 200 and fit["n_increments"] == int((truth >= 0).sum())
    assert np.all(np.abs(fit["Ds"] / np.array(hc.DS2) - 1.0) <= 0.10)
    assert np.all(np.abs(fit["M"] - np.array(hc.M2)) <= 0.03)
    acc = float((fit["state"][truth >= 0] == truth[truth >= 0]).mean())
    print("viterbi accuracy", acc)
    assert acc >= 0.95
    assert fit["gamma"].shape == (len(truth), 2) and fit["state"].shape == fit["state_posterior"].shape == (len(truth),)
    assert abs(fit["occupancy"].sum() - 1.0) <= 1e-12 and fit["Ds"][0] < fit["Ds"][1]
    assert fit["bic"] == -2.0 * fit["loglik"] + 5 * math.log(fit["n_increments"])


def test_loglik_never_decreases(fit200):
    tr = fit200[0]["loglik_trace"]
    assert len(tr) == fit200[0]["n_iter"] >= 3
    assert np.all(np.diff(tr) >= -1e-9 * np.abs(tr[1:]))


def test_one_state_fit_is_the_pooled_mle():
    pos, offsets, _ = hc.planted_set(40)
    fit = msd_mod.fit_diffusion_states(pos, offsets, 1, dt=0.5)
    q = np.concatenate([hc.increments(pos[a:b]) for a, b in zip(offsets[:-1], offsets[1:])])
    assert abs(fit["Ds"][0] / (q.sum() / (4.0 * len(q) * 0.5)) - 1.0) <= 1e-12
    assert fit["M"].tolist() == [[1.0]] and fit["p0"].tolist() == [1.0] and (fit["state"] == 0).all()


def test_nan_track_is_excluded_and_counted():
    pos, offsets, _ = hc.planted_set(40)
    bad = np.array(pos)
    bad[offsets[3] + 2, 0] = np.nan
    fit = msd_mod.fit_diffusion_states(bad, offsets, 2)
    assert fit["n_tracks_used"] == 39 and np.isfinite(fit["Ds"]).all() and np.isfinite(fit["loglik"])
    assert np.isnan(fit["gamma"][offsets[3]:offsets[4]]).all() and not np.isnan(fit["gamma"][offsets[4]:]).any()
    assert fit["n_increments"] == len(pos) - 40 - (offsets[4] - offsets[3] - 1)


def test_tensors_in_tensors_out_and_posteriors():
    pos, offsets, truth = hc.planted_set(40)
    post = msd_mod.hmm_posteriors(torch.from_numpy(np.array(pos)), torch.from_numpy(np.array(offsets)), hc.DS2, hc.M2)
    assert all(torch.is_tensor(x) for x in post.values())
    assert float((post["state"].numpy()[truth >= 0] == truth[truth >= 0]).mean()) >= 0.95
    arr = msd_mod.hmm_posteriors(pos, offsets, hc.DS2, hc.M2, p0=hc.stationary(hc.M2))
    assert np.allclose(arr["gamma"], post["gamma"].numpy(), rtol=0, atol=1e-12, equal_nan=True)


def test_argument_checks():
    pos, offsets, _ = hc.planted_set(40)
    for kw in ({"K": 0}, {"K": 9}, {"K": 2, "dt": 0.0}, {"K": 2, "sigma2": -1.0}, {"K": 2, "max_iter": 0},
               {"K": 2, "min_var": 0.0}, {"K": 2, "init": {"v": 1}}, {"K": 2, "init": {"Ds": [1.0]}}):
        with pytest.raises(ValueError):
            msd_mod.fit_diffusion_states(pos, offsets, **kw)
    with pytest.raises(ValueError):
        msd_mod.fit_diffusion_states(pos, offsets[:-1], 2)
    movie = torch.zeros(4, 16, 16)
    for states in ({"K": 2, "penalty": 1.0}, {"sigma2": 0.0}, 2):
        with pytest.raises(ValueError, match="states"):
            trk.estimate_track_diffusion(movie, torch.nn.Identity(), 2, states=states)
