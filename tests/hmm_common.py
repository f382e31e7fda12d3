"""The inputs and the two oracles shared by tests/test_hmm.py (CPU) and tests/test_hmm_gpu.py: the hidden Markov model over the
squared increments of a set of tracks, written from include/mivit_hip.h (mivit_hmm_estep, mivit_hmm_viterbi) and not from
helpers/msd.py.

Oracle (a), oracle_enumerate: BY DEFINITION.  For a track of at most 10 increments and K <= 3 every one of the K^T state
paths gets its probability pi[s_0] prod A[s_t][s_t+1] prod N(q_t; v_s_t) in float64, and math.fsum over the paths gives the
likelihood, gamma, xi and the most probable path.  No forward-backward at all.

Oracle (b), oracle_logdomain: an UNSCALED forward-backward and Viterbi in the log domain (np.logaddexp), for tracks of any
length.  It shares neither the scaling nor the underflow guard with the kernel.

Tolerance (HMM_TOL = 1e-10; absolute on gamma, relative to 1 + |x| on xi, g_sum, gq_sum, g_first and loglik).  The kernel
and its numpy restatement run the same operations in the same order; the only ones in which they may differ are exp (one per
state and increment) and log (one per increment), at about 1 ulp.  A prototype of the recurrence that perturbed every exp by
+-2.2e-16 relative at random moved gamma by at most 8.4e-15 and the statistics by at most 3.7e-15 relative, on tracks of up
to 4096 rows: the scaling renormalises alpha and beta at every step, so the errors do not compound along a track.  1e-10
leaves four orders of margin over that.  Oracle (b) works on log-probabilities of magnitude up to about 1e3 on the 513-row
tracks below (5e3 on the track with the large step), each rounded to 1.1e-16 relative, 1e-13 absolute, over at most 512
steps: about 2e-12 on a log-probability if the errors add as a random walk, which is the relative error of a posterior; 1e-10
still leaves a factor of 50.  Oracle (a) multiplies at most 21 factors per path and sums exactly: 3e-15.

What lets state be compared on EVERY row: tests/test_hmm.py asserts that the two largest gamma of every row of the common set
differ by at least MIN_GAP = 1e-6 under every parameter set, four orders above HMM_TOL, and that on the tracks given to
oracle (a) the best and the second-best path differ by at least MIN_GAP in log-probability."""
import functools
import itertools
import math

import numpy as np

HMM_TOL = 1e-10
MIN_GAP = 1e-6
V_WIDEST = 4.0                                                             # the largest v of any parameter set below
LOG_2PI = math.log(2.0 * math.pi)
FIXED_LENGTHS = (0, 1, 2, 3, 9, 64, 65, 513)
DS2, M2 = (0.05, 1.0), ((0.95, 0.05), (0.1, 0.9))
DS3, M3 = (0.02, 0.2, 2.0), ((0.9, 0.07, 0.03), (0.05, 0.9, 0.05), (0.02, 0.08, 0.9))


def stationary(M):
    M = np.asarray(M, np.float64)
    w, vec = np.linalg.eig(M.T)
    p = np.real(vec[:, np.argmin(np.abs(w - 1.0))])
    return p / p.sum()


def switching_track(rng, rows, Ds, M, dt=1.0):
    """A track of `rows` rows whose state follows the chain M from its stationary distribution -> (positions [rows, 2], the
    state of every increment [rows - 1])."""
    M, K = np.asarray(M, np.float64), len(Ds)
    s = np.zeros(max(rows - 1, 0), np.int64)
    for t in range(rows - 1):
        s[t] = rng.choice(K, p=stationary(M) if t == 0 else M[s[t - 1]])
    steps = rng.standard_normal((rows - 1, 2)) * np.sqrt(2.0 * np.asarray(Ds, np.float64)[s] * dt)[:, None]
    return np.concatenate([np.zeros((1, 2)), np.cumsum(steps, axis=0)]) + 20.0, s


def _stack(tracks):
    pos = np.ascontiguousarray(np.concatenate(tracks, axis=0))
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    pos.setflags(write=False)
    offsets.setflags(write=False)
    return pos, offsets


@functools.lru_cache(maxsize=None)
def common_tracks():
    """-> (pos [N, 2] float64, offsets [27] int64), read-only: 26 tracks, not a multiple of 8."""
    rng = np.random.default_rng(20241019)
    tracks = []
    for L in FIXED_LENGTHS:
        steps = rng.standard_normal((L, 2)) * math.sqrt(2.0 * 0.3)
        tracks.append(np.cumsum(steps, axis=0) + 20.0)
    tracks.append(np.full((20, 2), 7.25))                                  # never moves: q = 0
    big = np.cumsum(rng.standard_normal((20, 2)) * math.sqrt(2.0 * 0.3), axis=0) + 20.0
    big[10:, 0] += math.sqrt(1e4 * V_WIDEST)                               # one step of q = 1e4 * the widest v
    tracks.append(big)
    for rows in (11, 11, 20, 37, 50, 64, 90, 120):
        tracks.append(switching_track(rng, rows, DS2, M2)[0])
    for rows in (10, 11, 25, 40, 66, 100, 120, 30):
        tracks.append(switching_track(rng, rows, DS3, M3)[0])
    tracks.insert(4, tracks.pop(0))                                        # the empty track in the middle of the batch
    assert len(tracks) == 26
    return _stack(tracks)


@functools.lru_cache(maxsize=None)
def parameter_sets():
    """-> {name: (v [K], A [K, K], pi [K])}, float64 and read-only: v is the per-axis increment variance 2 D of each state."""
    rng = np.random.default_rng(7)
    A8 = rng.dirichlet(np.ones(8), size=8) * 0.5 + 0.5 * np.eye(8)
    sets = {
        "K1": (np.array([0.6]), np.ones((1, 1)), np.ones(1)),
        "K2": (2.0 * np.array(DS2), np.array(M2), stationary(M2)),
        "K3": (2.0 * np.array(DS3), np.array(M3), np.array([0.5, 0.3, 0.2])),
        "K8": (np.geomspace(0.02, V_WIDEST, 8), A8 / A8.sum(axis=1, keepdims=True), rng.dirichlet(np.ones(8))),
        "K2_identity": (2.0 * np.array(DS2), np.eye(2), np.array([0.5, 0.5])),
    }
    for v, A, pi in sets.values():
        for a in (v, A, pi):
            a.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def planted_set(n_tracks, seed=5):
    """The fit's input: n_tracks tracks of 20 to 120 rows under (DS2, M2) -> (pos, offsets, truth [N]: the state of the
    increment that starts at each row, -1 on a track's last row)."""
    rng = np.random.default_rng(seed)
    tracks, truth = [], []
    for _ in range(n_tracks):
        p, s = switching_track(rng, int(rng.integers(20, 121)), DS2, M2)
        tracks.append(p)
        truth.append(np.concatenate([s, [-1]]))
    pos, offsets = _stack(tracks)
    truth = np.concatenate(truth)
    truth.setflags(write=False)
    return pos, offsets, truth


def increments(p):
    d = np.diff(np.asarray(p, np.float64), axis=0)
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


def _log_density(q, v):
    """log of the density of an increment of squared length q in a state of per-axis variance v, [T, K]."""
    return -q[:, None] / (2.0 * v[None, :]) - np.log(2.0 * math.pi * v)[None, :]


def oracle_enumerate(p, v, A, pi):
    """One track [rows, 2] of 1 .. 10 increments, K <= 3 -> dict: loglik, gamma [T, K], xi [K, K], g_sum, gq_sum, g_first [K],
    path [T] (the most probable), logp (its log-probability, -T log(2 pi) included), gap (to the second-best path)."""
    q = increments(p)
    T, K = len(q), len(v)
    assert 1 <= T <= 10 and K <= 3
    paths = np.array(list(itertools.product(range(K), repeat=T)), np.int64)               # [K^T, T]
    dens = np.exp(-q[:, None] / (2.0 * v[None, :])) / (2.0 * math.pi * v[None, :])         # [T, K]
    prob = pi[paths[:, 0]] * dens[0, paths[:, 0]]
    with np.errstate(divide="ignore"):
        logprob = np.log(pi[paths[:, 0]]) + _log_density(q, v)[0, paths[:, 0]]
        for t in range(1, T):
            prob = prob * A[paths[:, t - 1], paths[:, t]] * dens[t, paths[:, t]]
            logprob = logprob + np.log(A[paths[:, t - 1], paths[:, t]]) + _log_density(q, v)[t, paths[:, t]]
    like = math.fsum(prob)
    gamma = np.array([[math.fsum(prob[paths[:, t] == j]) for j in range(K)] for t in range(T)]) / like
    xi = np.array([[math.fsum(math.fsum(prob[(paths[:, t] == i) & (paths[:, t + 1] == j)]) for t in range(T - 1))
                    for j in range(K)] for i in range(K)]) / like
    order = np.argsort(-logprob, kind="stable")
    gap = float(logprob[order[0]] - logprob[order[1]]) if len(order) > 1 else math.inf
    return {"loglik": math.log(like), "gamma": gamma, "xi": xi, "g_sum": gamma.sum(axis=0), "gq_sum": (gamma * q[:, None]).sum(axis=0),
            "g_first": gamma[0], "path": paths[order[0]], "logp": float(logprob[order[0]]), "gap": gap}


def oracle_logdomain(p, v, A, pi):
    """One track of any length >= 2 rows -> the same dict as oracle_enumerate (without gap), by an unscaled log-domain
    forward-backward and Viterbi."""
    q = increments(p)
    T, K = len(q), len(v)
    with np.errstate(divide="ignore"):
        lA, lpi = np.log(A), np.log(pi)
    lb = _log_density(q, v)
    la, lbeta = np.zeros((T, K)), np.zeros((T, K))
    la[0] = lpi + lb[0]
    for t in range(1, T):
        la[t] = np.logaddexp.reduce(la[t - 1][:, None] + lA, axis=0) + lb[t]
    for t in range(T - 2, -1, -1):
        lbeta[t] = np.logaddexp.reduce(lA + (lb[t + 1] + lbeta[t + 1])[None, :], axis=1)
    loglik = float(np.logaddexp.reduce(la[T - 1]))
    gamma = np.exp(la + lbeta - loglik)
    xi = np.zeros((K, K))
    for t in range(T - 1):
        xi += np.exp(la[t][:, None] + lA + (lb[t + 1] + lbeta[t + 1])[None, :] - loglik)
    delta, back = lpi + lb[0], np.zeros((T, K), np.int64)
    for t in range(1, T):
        cand = delta[:, None] + lA
        back[t] = np.argmax(cand, axis=0)
        delta = cand[back[t], np.arange(K)] + lb[t]
    path = np.zeros(T, np.int64)
    path[T - 1] = int(np.argmax(delta))
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return {"loglik": loglik, "gamma": gamma, "xi": xi, "g_sum": gamma.sum(axis=0), "gq_sum": (gamma * q[:, None]).sum(axis=0),
            "g_first": gamma[0], "path": path, "logp": float(np.max(delta))}


def close(got, want, what):
    """The statistics' tolerance: HMM_TOL relative to 1 + |x|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / (1.0 + np.abs(want))
    assert got.shape == want.shape and np.all(err <= HMM_TOL), (what, float(np.max(err)) if err.size else 0.0)
