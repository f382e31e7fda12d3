"""Shared by tests/test_fbm_ml.py (CPU) and tests/test_fbm_ml_gpu.py: the structure function of exposure-averaged fractional
Brownian motion at 50 digits (decimal) and by quadrature, the dense fp64 statement of the likelihood of
helpers/msd.estimate_anomalous_ml (the explicit matrix, np.linalg.slogdet and solve), a drawer of tracks by Cholesky of the
model covariance, and the batch of ranges on which the kernel (csrc/fbm_ml.hip) is held against the dense statement and the
numpy restatement.

The bars of the kernel against the restatement (BARS) are the issue's: four times the last bracket of the search (2.6e-5
in alpha, 2.2e-4 in log2 D) for the estimates, because an arg-min tie may flip between the two, and the flatness of the
likelihood across that bracket for loglik and the bars; status and n_increments are equal."""
from decimal import Decimal, getcontext

import numpy as np

from likelihood_common import close, usable_rows  # noqa: F401  (one home; the tests reach them through this module)

BARS = {"alpha": 1e-4, "D": 1e-3, "loglik": 1e-5, "alpha_std": 1e-2, "D_std": 1e-2}
LOGLIK_BAR = 1e-9             # against the dense statement, relative


def S_exact(alpha, lag, E):
    """the closed form of the structure function in decimal arithmetic at 50 digits, rounded to a float"""
    getcontext().prec = 50
    return float(_S_decimal(alpha, lag, E))


def S_quadrature(alpha, lag, E, n=2000):
    """the double integral of |lag + s - t|^alpha over the exposure, s, t in [0, E], by the midpoint rule on n x n cells,
    divided by E^2 (the average).  At lag 0 the integrand has its kink along the diagonal, where the midpoint of a cell says
    0 and costs 3e-4 at alpha = 0.05: the n diagonal cells take their own average instead, the elementary integral of
    |s - t|^alpha over a square of side h, 2 h^alpha / ((alpha + 1) (alpha + 2))."""
    h = E / n
    u = (np.arange(n) + 0.5) * h
    cells = np.abs(lag + u[:, None] - u[None, :]) ** alpha
    if lag == 0:
        cells[np.arange(n), np.arange(n)] = 2.0 * h ** alpha / ((alpha + 1.0) * (alpha + 2.0))
    return float(cells.mean())


def covariance(f, v, alpha, D, dt, E):
    """the covariance of the increments of one axis: f [m + 1] frames, v [m + 1] variances -> [m, m]; S at 50 digits, the
    four terms added in decimal arithmetic before the rounding"""
    getcontext().prec = 50
    f = [int(x) for x in f]
    m = len(f) - 1
    memo = {}

    def S(lag):
        lag = abs(lag)
        if lag not in memo:
            memo[lag] = _S_decimal(alpha, lag, E)
        return memo[lag]

    C = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            C[i, j] = C[j, i] = D * dt * float(S(f[i + 1] - f[j]) + S(f[i] - f[j + 1]) - S(f[i + 1] - f[j + 1]) - S(f[i] - f[j]))
    v = np.asarray(v, np.float64)
    return C + np.diag(v[:-1] + v[1:]) - np.diag(v[1:-1], 1) - np.diag(v[1:-1], -1)


def _S_decimal(alpha, lag, E):
    a, t, e = Decimal(float(alpha)), Decimal(abs(int(lag))), Decimal(float(E))
    if e == 0:
        return t ** a if t else Decimal(0)
    a12 = (a + 1) * (a + 2)
    if t == 0:
        return 2 * e ** a / a12
    p = a + 2
    far = abs(t - e)
    return ((t + e) ** p + (far ** p if far else Decimal(0)) - 2 * t ** p) / (e * e * a12)


def dense_loglik(X, v, f, alpha, D, dt, E):
    """log L of one track at (alpha, D) by dense linear algebra: X [m + 1, 2], v [m + 1, 2], f [m + 1] (all rows usable)"""
    d = np.diff(X, axis=0)
    total = 0.0
    for ax in (0, 1):
        C = covariance(f, v[:, ax], alpha, D, dt, E)
        sign, logdet = np.linalg.slogdet(C)
        if sign <= 0:
            return -np.inf
        total += logdet + d[:, ax] @ np.linalg.solve(C, d[:, ax]) + len(d) * np.log(2.0 * np.pi)
    return -0.5 * total


def draw(rng, n_tracks, rows, alpha, D, v0, dt=1.0, E=1.0, frames=None, mixed=True):
    """n_tracks tracks of `rows` observed rows each, drawn from the model: per axis the increments between the observed
    frames are L z with L the Cholesky factor of their covariance without noise, the rows are their running sum from a
    random start plus noise of each row's own variance.  frames: None (consecutive) or the number of frames the rows are
    spread over.  Variances v0 * {0.25 or 1.75} per row and axis (mixed), or v0.
    -> (pos [N, 2], var [N, 2], frames [N] int64, offsets [n_tracks + 1] int64)"""
    pos, var, fr = [], [], []
    for _ in range(n_tracks):
        if frames is None:
            f = np.arange(rows)
        else:
            f = np.sort(np.concatenate([[0], 1 + rng.permutation(int(frames) - 1)[:rows - 1]]))
        L = np.linalg.cholesky(covariance(f, np.zeros(rows), alpha, D, dt, E))
        walk = np.concatenate([np.zeros((1, 2)), np.cumsum(L @ rng.standard_normal((rows - 1, 2)), axis=0)])
        v = v0 * (rng.choice([0.25, 1.75], (rows, 2)) if mixed else np.ones((rows, 2)))
        pos.append(rng.uniform(10.0, 50.0, (1, 2)) + walk + rng.standard_normal((rows, 2)) * np.sqrt(v))
        var.append(v)
        fr.append(f)
    return (np.concatenate(pos), np.concatenate(var), np.concatenate(fr).astype(np.int64),
            (np.arange(n_tracks + 1) * rows).astype(np.int64))


# ----------------------------------------------------------------------------------------------------------------------
# the batch of the kernel tests
# ----------------------------------------------------------------------------------------------------------------------
BATCH_DT = 0.5
MAX_ROWS = 129                # ops.FBM_ML_MAX_ROWS (tests/test_fbm_ml.py holds the two equal)


def batch():
    """-> dict: pos [N, 2], var [N, 2], frames [N] int32, use [N] bool, offsets [n + 1] int64, names [n], alpha, D [n] (the
    parameters at which the first entry is asked for the likelihood: the truths of the draw).  0 .. 4 usable rows, 5, 33, 64,
    65, 129 = MAX_ROWS and MAX_ROWS + 1 rows, a frame gap of 1000, a span over the limit, NaN positions, negative and infinite
    variances, use masks, truths alpha 0.3, 1.0, 1.7, a motionless range, one with huge noise, and small ordinary ranges."""
    rng = np.random.default_rng(2027)
    parts, names, alphas, Ds = [], [], [], []

    def add(name, rows, alpha=1.0, D=0.05, v0=0.02, frames=None, edit=None, E=1.0):
        if rows >= 2:
            p, v, f, _ = draw(rng, 1, rows, alpha, D, v0, BATCH_DT, E, frames)
        else:
            p, v, f = np.full((rows, 2), 20.0), np.full((rows, 2), v0), np.arange(rows, dtype=np.int64)
        u = np.ones(rows, bool)
        if edit:
            edit(p, v, f, u)
        parts.append((p, v, f + 3 * len(parts), u))                       # frames need not start at 0
        names.append(name)
        alphas.append(alpha)
        Ds.append(D)

    def still(p, v, f, u):
        p[:] = p[0]

    def gap(p, v, f, u):
        f[len(f) // 2:] += 1000

    for L in (0, 1, 2, 3, 4):
        add(f"{L} rows", L)
    add("every row unusable", 6, edit=lambda p, v, f, u: u.__setitem__(slice(None), False))
    add("3 usable of 7", 7, edit=lambda p, v, f, u: u.__setitem__(slice(3, None), False))
    add("4 usable of 9", 9, edit=lambda p, v, f, u: u.__setitem__(slice(0, 5), False))
    for rows, alpha in ((5, 1.0), (33, 0.3), (64, 1.7), (65, 1.0), (MAX_ROWS, 0.3), (MAX_ROWS + 1, 1.0)):
        add(f"{rows} rows", rows, alpha=alpha)
    add("more usable rows than the limit among unusable ones", MAX_ROWS + 40, edit=lambda p, v, f, u: u.__setitem__(slice(0, 30, 3), False))
    add("a gap of 1000 frames", 24, alpha=1.7, edit=gap)
    add("a span over the limit", 12, edit=lambda p, v, f, u: f.__setitem__(slice(6, None), f[6:] + 1300))
    add("two rows, a span over the limit", 2, edit=lambda p, v, f, u: f.__setitem__(1, 5000))
    add("NaN position", 14, alpha=0.3, edit=lambda p, v, f, u: p.__setitem__((4, 1), np.nan))
    add("inf position", 14, edit=lambda p, v, f, u: p.__setitem__((0, 0), np.inf))
    add("negative variance", 14, alpha=1.7, edit=lambda p, v, f, u: v.__setitem__((5, 0), -1e-3))
    add("infinite variance", 14, edit=lambda p, v, f, u: v.__setitem__((13, 1), np.inf))
    add("use mask", 30, alpha=0.3, edit=lambda p, v, f, u: u.__setitem__(slice(2, None, 4), False))
    add("gaps 20 of 39", 20, alpha=1.7, frames=39)
    add("gaps and a use mask", 33, frames=50, edit=lambda p, v, f, u: u.__setitem__(slice(2, None, 5), False))
    add("motionless", 12, edit=still)
    add("motionless, no variance", 12, edit=lambda p, v, f, u: (still(p, v, f, u), v.__setitem__(slice(None), 0.0)))
    add("huge noise", 40, D=0.01, v0=25.0)
    add("no variance", 30, alpha=1.7, edit=lambda p, v, f, u: v.__setitem__(slice(None), 0.0))
    k = 0
    while len(parts) < 40:
        add(f"ordinary {k}", int(rng.integers(6, 40)), alpha=(0.3, 1.0, 1.7)[k % 3], D=float(10.0 ** rng.uniform(-2.0, -0.5)),
            v0=float(10.0 ** rng.uniform(-3, -1.5)))
        k += 1
    lengths = [len(p[0]) for p in parts]
    return {"pos": np.ascontiguousarray(np.concatenate([p[0] for p in parts])),
            "var": np.ascontiguousarray(np.concatenate([p[1] for p in parts])),
            "frames": np.concatenate([p[2] for p in parts]).astype(np.int32),
            "use": np.concatenate([p[3] for p in parts]),
            "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "names": names,
            "alpha": np.array(alphas), "D": np.array(Ds)}


