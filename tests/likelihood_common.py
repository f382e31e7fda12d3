"""Shared by tests/test_likelihood.py (CPU) and tests/test_likelihood_gpu.py: tracks drawn from the model of
helpers/msd.estimate_diffusion_ml by a construction that does not use its covariance, a dense fp64 statement of its
likelihood, and the batch of ranges on which the kernel (csrc/likelihood.hip) is held against the numpy restatement.

The draw.  Per frame and axis a Brownian particle moves by B ~ N(0, s), s = 2 D dt, and a camera that exposes over the whole
frame sees its time average, which lies A beyond the frame's starting point with var A = s / 3 and cov(A, B) = s / 2 (the
integral of a Wiener process): A = B / 2 + sqrt(s / 12) N(0, 1).  The observed row is start + A + localisation noise of the
row's own variance.  Its increments have the variance s (1 - 2 R) + v_k + v_{k+1} and the neighbour covariance R s - v_{k+1}
with R = 1 / 6: the model, arrived at from the other side.  Rows are then dropped to make gaps.

The bars of the kernel against the restatement (BARS) are the issue's: the two differ in log and exp2, the cost is flat to
rounding within about 1e-7 of D, so D agrees to 1e-6, D_std to 1e-5 and loglik (second order in D at the optimum) to 1e-10
relative; status and n_increments are equal."""
import numpy as np

R_FRAME = 1.0 / 6.0
BARS = {"D": 1e-6, "D_std": 1e-5, "loglik": 1e-10}


def draw(rng, n_tracks, rows, D, v0, dt=1.0, frames=None, mixed=True):
    """n_tracks tracks of `rows` observed rows each, exposure over the whole frame (R = 1/6).  frames: None (consecutive) or
    the number of frames the observed rows are spread over (each track keeps its first and a random choice of the others).
    Row variances v0 * {0.25 or 1.75}, chosen per row and axis (mixed), or v0.
    -> (pos [N, 2], var [N, 2], frames [N] int64, offsets [n_tracks + 1] int64)"""
    F = rows if frames is None else int(frames)
    s = 2.0 * D * dt
    B = rng.standard_normal((n_tracks, F, 2)) * np.sqrt(s)
    A = B / 2.0 + rng.standard_normal((n_tracks, F, 2)) * np.sqrt(s / 12.0)
    start = np.concatenate([np.zeros((n_tracks, 1, 2)), np.cumsum(B, axis=1)[:, :-1]], axis=1) + rng.uniform(10.0, 50.0, (n_tracks, 1, 2))
    if F == rows:
        keep = np.tile(np.arange(F), (n_tracks, 1))
    else:
        keep = np.stack([np.sort(np.concatenate([[0], 1 + rng.permutation(F - 1)[:rows - 1]])) for _ in range(n_tracks)])
    seen = np.take_along_axis(start + A, keep[:, :, None], axis=1)
    var = v0 * (rng.choice([0.25, 1.75], (n_tracks, rows, 2)) if mixed else np.ones((n_tracks, rows, 2)))
    pos = seen + rng.standard_normal((n_tracks, rows, 2)) * np.sqrt(var)
    return (pos.reshape(-1, 2), var.reshape(-1, 2), keep.reshape(-1).astype(np.int64),
            (np.arange(n_tracks + 1) * rows).astype(np.int64))


def dense_loglik(X, v, f, D, dt, R):
    """log L of one track at D by dense linear algebra: X [m, 2], v [m, 2], f [m] frames (all rows usable)."""
    d, g = np.diff(X, axis=0), np.diff(f).astype(np.float64)
    m1 = len(d)
    total = 0.0
    for ax in (0, 1):
        C = np.diag(2.0 * D * dt * (g - 2.0 * R) + v[:-1, ax] + v[1:, ax])
        if m1 > 1:
            b = 2.0 * R * D * dt - v[1:-1, ax]
            C = C + np.diag(b, 1) + np.diag(b, -1)
        sign, logdet = np.linalg.slogdet(C)
        if sign <= 0:
            return -np.inf
        total += logdet + d[:, ax] @ np.linalg.solve(C, d[:, ax]) + m1 * np.log(2.0 * np.pi)
    return -0.5 * total


def d_ref(X, f, dt):
    d, g = np.diff(X, axis=0), np.diff(f)
    return (d * d).sum() / (4.0 * dt * g.sum())


# ----------------------------------------------------------------------------------------------------------------------
# the batch of the kernel tests: 67 ranges
# ----------------------------------------------------------------------------------------------------------------------
BATCH_DT, BATCH_R, BATCH_N = 0.5, R_FRAME, 67
LONG_ROWS = 300                # the kernel stages nothing (it reads global memory every pass): 300 rows, several cache lines of every array


def batch():
    """-> dict: pos [N, 2], var [N, 2], frames [N] int32, use [N] bool, offsets [68] int64, names [67].  The edge cases of
    tests/test_likelihood.py, a range of LONG_ROWS rows, ranges with gaps, ranges with unusable rows, and seeded ordinary
    ranges of 4 .. 60 rows up to 67."""
    rng = np.random.default_rng(20260)
    parts, names = [], []

    def add(name, rows, D=0.05, v0=0.02, frames=None, edit=None):
        if rows:
            p, v, f, _ = draw(rng, 1, rows, D, v0, BATCH_DT, frames)
        else:
            p, v, f = np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0, np.int64)
        u = np.ones(rows, bool)
        if edit:
            edit(p, v, f, u)
        parts.append((p, v, f + 3 * len(parts), u))                       # frames need not start at 0
        names.append(name)

    def still(p, v, f, u):
        p[:] = p[0]

    for L in (0, 1, 2, 3):
        add(f"{L} rows", L)
    add("every row unusable", 9, edit=lambda p, v, f, u: u.__setitem__(slice(None), False))
    add("one usable row", 6, edit=lambda p, v, f, u: u.__setitem__(slice(1, None), False))
    add("NaN position", 12, edit=lambda p, v, f, u: p.__setitem__((4, 1), np.nan))
    add("inf position", 12, edit=lambda p, v, f, u: p.__setitem__((0, 0), np.inf))
    add("negative variance", 12, edit=lambda p, v, f, u: v.__setitem__((5, 0), -1e-3))
    add("NaN variance", 12, edit=lambda p, v, f, u: v.__setitem__((11, 1), np.nan))
    add("3 rows, NaN in the middle", 3, edit=lambda p, v, f, u: p.__setitem__((1, 0), np.nan))
    add("identical positions", 10, edit=still)
    add("identical positions, no variance", 10, edit=lambda p, v, f, u: (still(p, v, f, u), v.__setitem__(slice(None), 0.0)))
    add("no variance", 30, edit=lambda p, v, f, u: v.__setitem__(slice(None), 0.0))
    # rows that scatter by less than their stated noise (0.05 against a standard deviation of 0.11 .. 0.3): the cost rises with D
    add("immobile within its noise", 40, v0=0.05, edit=lambda p, v, f, u: (still(p, v, f, u), p.__setitem__(slice(1, None, 2), p[0] + 0.05)))
    add("long", LONG_ROWS, D=0.01, v0=0.04)
    for i, (rows, frames) in enumerate([(50, 70), (20, 39), (7, 30), (3, 9)]):
        add(f"gaps {rows} of {frames}", rows, frames=frames)
    for i, rows in enumerate((40, 17, 8, 5)):
        def drop(p, v, f, u, i=i):
            u[np.random.default_rng(i).permutation(len(u))[:len(u) // 3]] = False
        add(f"unusable rows {rows}", rows, edit=drop)
    add("gaps and unusable rows", 33, frames=50, edit=lambda p, v, f, u: u.__setitem__(slice(2, None, 5), False))
    k = 0
    while len(parts) < BATCH_N:
        add(f"ordinary {k}", int(rng.integers(4, 61)), D=float(10.0 ** rng.uniform(-2.5, -0.5)), v0=float(10.0 ** rng.uniform(-3, -1)))
        k += 1
    lengths = [len(p[0]) for p in parts]
    return {"pos": np.ascontiguousarray(np.concatenate([p[0] for p in parts])),
            "var": np.ascontiguousarray(np.concatenate([p[1] for p in parts])),
            "frames": np.concatenate([p[2] for p in parts]).astype(np.int32),
            "use": np.concatenate([p[3] for p in parts]),
            "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "names": names}


def usable_rows(b, k):
    """(X, v, f) of the usable rows of range k of a batch (this one's, or that of fbm_ml_common or confined_ml_common)"""
    a, e = int(b["offsets"][k]), int(b["offsets"][k + 1])
    with np.errstate(invalid="ignore"):
        ok = b["use"][a:e] & np.isfinite(b["pos"][a:e]).all(1) & ((b["var"][a:e] >= 0) & (b["var"][a:e] < np.inf)).all(1)
    return b["pos"][a:e][ok], b["var"][a:e][ok], b["frames"][a:e][ok].astype(np.int64)


def close(tol, relative=True):
    """equal where both are NaN, both the same infinity or exactly equal; within tol (relative or absolute) elsewhere"""
    def check(got, want, what=""):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN in other places"
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got - want) / (np.abs(want) if relative else 1.0)
            err = np.where((got == want) | np.isnan(want), 0.0, err)
        assert err.max(initial=0.0) <= tol, f"{what}: worst difference {err.max():.3g} > {tol:g} at {int(err.argmax())}"
    return check
