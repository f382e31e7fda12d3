"""Shared by tests/test_confined_ml.py (CPU) and tests/test_confined_ml_gpu.py: the dense fp64 statement of the likelihood
of helpers/msd.estimate_confinement_ml (the explicit mean and covariance of an Ornstein-Uhlenbeck process conditioned on its
first row, np.linalg.slogdet and solve), a drawer of tracks from the exact discretisation of the process, and the batch of
ranges on which the kernel (csrc/confined_ml.hip) is held against the numpy restatement."""
import numpy as np

from likelihood_common import close, usable_rows  # noqa: F401  (one home; the tests reach them through this module)

LOGLIK_BAR = 1e-9             # the restatement against the dense statement, relative (as fbm_ml_common.LOGLIK_BAR)
NESTING_BAR = 1e-8            # the log-likelihood at s2 = 1e9 D against estimate_diffusion_ml(blur=0), relative
SEARCH_LOSS_BAR = 1e-5        # -2 log L that the fixed search may lose to a polish of the dense likelihood

LAST_BRACKET_U = 16.0 * (4.0 / 7.0) ** 20     # the bracket that would follow the last round, in log2 D: 2.2e-4
LAST_BRACKET_W = 24.0 * (4.0 / 7.0) ** 20     # and in log2 s2: 3.3e-4

BARS = {"D_conf": 4.0 * LAST_BRACKET_U * np.log(2.0), "radius": 4.0 * LAST_BRACKET_W * np.log(2.0) / 2.0,
        "lambda": 4.0 * (LAST_BRACKET_U + LAST_BRACKET_W) * np.log(2.0), "loglik": 1e-9,
        "D_conf_std": 1e-2, "radius_std": 1e-2, "lambda_std": 1e-2, "corr": 1e-2, "centre_std": 1e-2}
"""The bars of the kernel against the restatement, relative but for corr.  Estimates: four times the last bracket of the
search, because an arg-min tie may flip between the two: D moves by a factor 2^(4 x 2.2e-4), a relative 6.1e-4; the radius
is sqrt(2 s2) and moves by half of 2^(4 x 3.3e-4), 4.6e-4; lambda = D / s2 by the sum, 1.5e-3.  loglik 1e-9 relative and the
error bars 1e-2 are the issue's.  The centre is a function of (D, s2): it is held to BARS["lambda"] times its standard
error, its sensitivity to the relaxation rate being of the order of its own uncertainty.

The fixed search against a polish of the dense likelihood by scipy's Nelder-Mead, started from the restatement's answer and
from the truth (tests/test_confined_ml.py::test_the_search_against_a_polish, 24 tracks with lambda dt <= 1): the worst loss
seen in -2 log L was 1.8e-08 against the bar SEARCH_LOSS_BAR = 1e-5."""


def dense_loglik(X, v, f, D, s2, dt, centre=None):
    """log L of one track under the Ornstein-Uhlenbeck model by dense linear algebra: X [m + 1, 2], v [m + 1, 2], f [m + 1]
    (all rows usable), conditioned on the first row (a diffuse prior on the start).  Per axis the rows k >= 1 have the mean
    c + e^{-lam t_k} (y_0 - c) and the covariance s2 (e^{-lam |t_j - t_k|} - e^{-lam (t_j + t_k)}) + e^{-lam (t_j + t_k)} v_0 +
    delta_jk v_k with t_k = dt (f_k - f_0).  centre (y, x), or None: each axis takes the generalised-least-squares centre."""
    lam = D / s2
    t = dt * (np.asarray(f, np.float64)[1:] - float(f[0]))
    m = len(t)
    total = 0.0
    for ax in (0, 1):
        y0, v0 = X[0, ax], v[0, ax]
        decay = np.exp(-lam * (t[:, None] + t[None, :]))
        C = s2 * (np.exp(-lam * np.abs(t[:, None] - t[None, :])) - decay) + decay * v0 + np.diag(v[1:, ax])
        sign, logdet = np.linalg.slogdet(C)
        if sign <= 0:
            return -np.inf
        e = np.exp(-lam * t)
        r0, h = X[1:, ax] - e * y0, -np.expm1(-lam * t)                   # the residual is r0 - h c
        Cr, Ch = np.linalg.solve(C, r0), np.linalg.solve(C, h)
        if centre is None:
            hh = h @ Ch
            quad = r0 @ Cr - ((h @ Cr) ** 2 / hh if hh > 0 else 0.0)
        else:
            r = r0 - h * centre[ax]
            quad = r @ np.linalg.solve(C, r)
        total += logdet + quad + m * np.log(2.0 * np.pi)
    return -0.5 * total


def draw(rng, n_tracks, rows, D, lam, v0, dt=1.0, frames=None, mixed=True, stationary=True):
    """n_tracks tracks of `rows` observed rows each from the exact discretisation of the Ornstein-Uhlenbeck process with
    s2 = D / lam about a random centre (lam = 0: free Brownian motion), started in the stationary law (or at the centre),
    plus noise of each row's own variance.  frames: None (consecutive) or the number of frames the rows are spread over.
    Variances v0 * {0.25 or 1.75} per row and axis (mixed), or v0.
    -> (pos [N, 2], var [N, 2], frames [N] int64, offsets [n_tracks + 1] int64, centres [n_tracks, 2])"""
    pos, var, fr, cen = [], [], [], []
    for _ in range(n_tracks):
        if frames is None:
            f = np.arange(rows)
        else:
            f = np.sort(np.concatenate([[0], 1 + rng.permutation(int(frames) - 1)[:rows - 1]]))
        c = rng.uniform(10.0, 50.0, 2)
        x = np.zeros((rows, 2))
        if lam > 0:
            s2 = D / lam
            x[0] = rng.standard_normal(2) * np.sqrt(s2) if stationary else 0.0
            for k in range(1, rows):
                phi = np.exp(-lam * dt * (f[k] - f[k - 1]))
                x[k] = phi * x[k - 1] + np.sqrt(s2 * (1.0 - phi * phi)) * rng.standard_normal(2)
        else:
            for k in range(1, rows):
                x[k] = x[k - 1] + np.sqrt(2.0 * D * dt * (f[k] - f[k - 1])) * rng.standard_normal(2)
        v = v0 * (rng.choice([0.25, 1.75], (rows, 2)) if mixed else np.ones((rows, 2)))
        pos.append(c + x + rng.standard_normal((rows, 2)) * np.sqrt(v))
        var.append(v)
        fr.append(f)
        cen.append(c)
    return (np.concatenate(pos), np.concatenate(var), np.concatenate(fr).astype(np.int64),
            (np.arange(n_tracks + 1) * rows).astype(np.int64), np.array(cen))


# ----------------------------------------------------------------------------------------------------------------------
# the constructed ranges of the statuses
# ----------------------------------------------------------------------------------------------------------------------
def straight_walk(rng, rows=80, speed=1.0, step=0.3, noise=0.02):
    """a straight noisy walk: a Brownian walk (steps of sd `step`) on a path that runs straight away and gains speed by a
    quarter over its length, which no well can imitate (a pull towards a centre only ever slows a particle down), seen through
    a little noise: the likelihood rises with s2 beyond the bracket (status 2)"""
    t = np.arange(rows, dtype=np.float64)[:, None]
    path = (speed * t) * (1.0 + 0.125 * t / rows) * np.array([[1.0, 0.5]])
    walk = np.cumsum(rng.standard_normal((rows, 2)) * step, axis=0)
    return np.array([[20.0, 30.0]]) + path + walk + rng.standard_normal((rows, 2)) * noise, np.full((rows, 2), noise ** 2)


def white_noise(rng, rows=60, sd=0.5):
    """white noise about a point with rows of much smaller stated variance: the particle relaxes within a frame (status 3)"""
    return np.array([[20.0, 30.0]]) + rng.standard_normal((rows, 2)) * sd, np.full((rows, 2), 1e-4)


def identical(rows=12, v=0.01):
    """identical rows: D_ref = S_ref = 0, no candidate is accepted (status 4)"""
    return np.tile(np.array([[20.0, 30.0]]), (rows, 1)), np.full((rows, 2), v)


# ----------------------------------------------------------------------------------------------------------------------
# the batch of the kernel tests
# ----------------------------------------------------------------------------------------------------------------------
BATCH_DT = 0.5
MIN_STATUS_0 = 40


def batch():
    """-> dict: pos [N, 2], var [N, 2], frames [N] int32, use [N] bool, offsets [n + 1] int64, names [n], D, s2 [n], centre
    [n, 2] (the parameters at which mivit_track_confined_loglik is asked: the truths of the draw).  60 ranges: 0 .. 3 rows, 4
    rows (3 increments) and 5 rows (4 increments, the shortest accepted), unusable rows of every kind, use masks, gaps, the
    constructed ranges of statuses 2, 3 and 4, a range of 300 rows, a free walk, and ordinary ranges of 5 to 60 rows."""
    rng = np.random.default_rng(2031)
    parts, names, Ds, S2s, cens = [], [], [], [], []

    def add(name, rows, D=0.5, lam=0.6, v0=0.02, frames=None, edit=None, given=None):
        c = np.array([20.0, 20.0])
        if given is not None:
            p, v = given
            f = np.arange(len(p), dtype=np.int64)
        elif rows >= 2:
            p, v, f, _, c = draw(rng, 1, rows, D, lam, v0, BATCH_DT, frames)
            c = c[0]
        else:
            p, v, f = np.full((rows, 2), 20.0), np.full((rows, 2), v0), np.arange(rows, dtype=np.int64)
        u = np.ones(len(p), bool)
        if edit:
            edit(p, v, f, u)
        parts.append((p, v, f + 3 * len(parts), u))                       # frames need not start at 0
        names.append(name)
        Ds.append(D)
        S2s.append(D / lam if lam > 0 else 1e6)
        cens.append(c)

    for L in (0, 1, 2, 3, 4, 5):
        add(f"{L} rows", L)
    add("every row unusable", 8, edit=lambda p, v, f, u: u.__setitem__(slice(None), False))
    add("4 usable of 9", 9, edit=lambda p, v, f, u: u.__setitem__(slice(4, None), False))
    add("5 usable of 11", 11, edit=lambda p, v, f, u: u.__setitem__(slice(0, 6), False))
    add("NaN position", 24, edit=lambda p, v, f, u: p.__setitem__((4, 1), np.nan))
    add("inf position", 24, edit=lambda p, v, f, u: p.__setitem__((0, 0), np.inf))
    add("negative variance", 24, edit=lambda p, v, f, u: v.__setitem__((5, 0), -1e-3))
    add("infinite variance", 24, edit=lambda p, v, f, u: v.__setitem__((23, 1), np.inf))
    add("one zero variance", 24, edit=lambda p, v, f, u: v.__setitem__((7, 0), 0.0))
    add("no variance", 30, edit=lambda p, v, f, u: v.__setitem__(slice(None), 0.0))
    add("use mask", 40, edit=lambda p, v, f, u: u.__setitem__(slice(2, None, 4), False))
    add("gaps 30 of 59", 30, frames=59)
    add("gaps and a use mask", 45, frames=70, edit=lambda p, v, f, u: u.__setitem__(slice(2, None, 5), False))
    add("a gap of 1000 frames", 40, edit=lambda p, v, f, u: f.__setitem__(slice(20, None), f[20:] + 1000))
    add("straight walk", 60, given=straight_walk(rng))
    add("white noise", 60, given=white_noise(rng))
    add("identical rows", 12, given=identical())
    add("identical rows, no variance", 12, given=identical(v=0.0))
    add("300 rows", 300)
    add("free walk", 60, lam=0.0)
    add("huge noise", 60, v0=25.0)
    k = 0
    while len(parts) < 60:
        add(f"ordinary {k}", int(rng.integers(25, 61)) if k % 4 else int(rng.integers(5, 25)), D=float(10.0 ** rng.uniform(-1.5, 0.5)),
            lam=float(10.0 ** rng.uniform(-1.0, 0.2)), v0=float(10.0 ** rng.uniform(-3, -1.5)))
        k += 1
    lengths = [len(p[0]) for p in parts]
    return {"pos": np.ascontiguousarray(np.concatenate([p[0] for p in parts])),
            "var": np.ascontiguousarray(np.concatenate([p[1] for p in parts])),
            "frames": np.concatenate([p[2] for p in parts]).astype(np.int32),
            "use": np.concatenate([p[3] for p in parts]),
            "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "names": names,
            "D": np.array(Ds), "s2": np.array(S2s), "centre": np.ascontiguousarray(np.array(cens))}


