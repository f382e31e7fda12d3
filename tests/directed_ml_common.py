"""Shared by tests/test_directed_ml.py (CPU) and tests/test_directed_ml_gpu.py: directed tracks drawn by a construction that
does not use the model's covariance (likelihood_common.draw plus velocity x frame x dt), a dense fp64 statement of the
likelihood of helpers/msd.estimate_directed_ml (the covariance of likelihood_common.dense_loglik, the velocity profiled
with np.linalg.solve), and the batch of ranges on which the kernels (csrc/directed_ml.hip) are held against the numpy
restatement."""
import numpy as np

import likelihood_common as lc
from confined_ml_common import LOGLIK_BAR, SEARCH_LOSS_BAR  # noqa: F401  (the issue's bars; the tests reach them through this module)
from likelihood_common import close, usable_rows  # noqa: F401

R_FRAME = lc.R_FRAME

MOVED_BY_THE_D_BAR = {"velocity": 2.73e-07, "velocity_std": 5.01e-07}
BARS = dict(lc.BARS, velocity=10.0 * MOVED_BY_THE_D_BAR["velocity"], velocity_std=10.0 * MOVED_BY_THE_D_BAR["velocity_std"])
"""The bars of the kernel against the restatement.  D, D_std and loglik are those of likelihood_common.BARS (the same search:
the two implementations may settle on neighbouring grid points of a cost that is flat to rounding within about 1e-7 of D).
velocity (in units of velocity_std) and velocity_std (relative) are measured, not guessed: the D bar lets D move by a factor
e^{1e-6}, and over the status-0 ranges of the batch the restatement's profiled velocity then moves by at most 2.72e-07 of
its standard error and that standard error by at most 5.00e-07 of itself (C is a sum of terms between 1 / D and 1 / noise,
so velocity_std = C^{-1/2} can move by no more than half of what D moves by).  MOVED_BY_THE_D_BAR holds the two figures,
tests/test_directed_ml.py::test_what_the_D_bar_lets_the_velocity_move_by measures them again, and the bars are ten times
them, because the two implementations may sit several grid steps apart."""


def draw(rng, n_tracks, rows, D, v0, velocity, dt=1.0, frames=None, mixed=True):
    """likelihood_common.draw (exposure over the whole frame, R = 1/6) plus velocity x frame x dt; velocity [2] or [n_tracks,
    2] in pixels per unit of dt, (y, x) -> (pos [N, 2], var [N, 2], frames [N] int64, offsets [n_tracks + 1] int64)"""
    pos, var, fr, off = lc.draw(rng, n_tracks, rows, D, v0, dt, frames, mixed)
    vel = np.broadcast_to(np.asarray(velocity, np.float64), (n_tracks, 2))
    return pos + np.repeat(vel, rows, axis=0) * (fr[:, None] * dt), var, fr, off


def dense_fit(X, v, f, D, dt, R, velocity=None):
    """One track at D by dense linear algebra: X [m, 2], v [m, 2], f [m] frames (all rows usable); the covariance is that of
    likelihood_common.dense_loglik, the mean velocity x gap x dt.  velocity (y, x), or None: each axis takes the generalised-
    least-squares velocity b / c and the quadratic form loses b^2 / c -> (log L, velocity [2], its standard error [2])"""
    d, g = np.diff(X, axis=0), np.diff(f).astype(np.float64)
    m1, m = len(d), np.diff(f).astype(np.float64) * dt
    total, u, sd = 0.0, np.zeros(2), np.zeros(2)
    for ax in (0, 1):
        C = np.diag(2.0 * D * dt * (g - 2.0 * R) + v[:-1, ax] + v[1:, ax])
        if m1 > 1:
            b = 2.0 * R * D * dt - v[1:-1, ax]
            C = C + np.diag(b, 1) + np.diag(b, -1)
        sign, logdet = np.linalg.slogdet(C)
        if sign <= 0:
            return -np.inf, np.full(2, np.nan), np.full(2, np.nan)
        Cd, Cm = np.linalg.solve(C, d[:, ax]), np.linalg.solve(C, m)
        bb, cc = m @ Cd, m @ Cm
        u[ax], sd[ax] = bb / cc, 1.0 / np.sqrt(cc)
        if velocity is None:
            quad = d[:, ax] @ Cd - bb * bb / cc
        else:
            r = d[:, ax] - velocity[ax] * m
            quad = r @ np.linalg.solve(C, r)
        total += logdet + quad + m1 * np.log(2.0 * np.pi)
    return -0.5 * total, u, sd


# ----------------------------------------------------------------------------------------------------------------------
# the batch of the kernel tests
# ----------------------------------------------------------------------------------------------------------------------
BATCH_DT, BATCH_R = lc.BATCH_DT, lc.BATCH_R
LINE_VELOCITY = np.array([0.5, -1.0])          # times dt = 0.5 and whole frames: every position is exact in binary
FAST = 1000.0                                  # |v| dt of the fast range in step standard deviations
MIN_STATUS_0 = 45


def batch():
    """-> dict: pos [N, 2], var [N, 2], frames [N] int32, use [N] bool, offsets [n + 1] int64, names [n], D [n], velocity [n, 2]
    (the parameters at which mivit_track_directed_loglik is asked).  The 67 ranges of likelihood_common.batch(), each moved
    by a seeded velocity of its own, and then: a straight line with zero variances (D_ref = 0 and no candidate is accepted), a
    straight line within its stated noise (status 2 with a finite velocity), a range with |v| dt = 1000 step standard
    deviations, a directed range of exactly 3 rows (the smallest that reaches the branch of the recurrence that is not the
    first), a directed range of 300 rows, and directed ranges with gaps and with one zero variance."""
    b = lc.batch()
    rng = np.random.default_rng(20261)
    n0 = len(b["names"])
    lengths = np.diff(b["offsets"])
    vel = rng.normal(0.0, 1.0, (n0, 2))
    pos = b["pos"] + np.repeat(vel, lengths, axis=0) * (b["frames"].astype(np.float64)[:, None] * BATCH_DT)
    parts, names, vels, Ds = [], [], list(vel), [0.05] * n0

    def add(name, p, v, f, velocity, D=0.05):
        parts.append((p, v, f + 3 * (n0 + len(parts)), np.ones(len(p), bool)))
        names.append(name)
        vels.append(np.asarray(velocity, np.float64))
        Ds.append(D)

    def line(rows):
        f = np.arange(rows, dtype=np.int64)
        return np.array([[20.0, 30.0]]) + LINE_VELOCITY[None, :] * (f[:, None] * BATCH_DT), f

    p, f = line(12)
    add("straight line, no variance", p, np.zeros((12, 2)), f, LINE_VELOCITY)
    p, f = line(40)
    p[1::2] += 0.05                            # scatters by 0.05 against stated standard deviations of 0.11 .. 0.3
    add("straight line within its noise", p, 0.05 * rng.choice([0.25, 1.75], (40, 2)), f, LINE_VELOCITY)
    step = np.sqrt(2.0 * 0.05 * BATCH_DT)
    fast = FAST * step / BATCH_DT * np.array([0.6, -0.8])
    p, v, f, _ = draw(rng, 1, 30, 0.05, 0.02, fast, BATCH_DT)
    add("fast", p, v, f, fast)
    for name, rows, frames in (("3 rows, directed", 3, None), ("300 rows, directed", lc.LONG_ROWS, None), ("directed, gaps 25 of 40", 25, 40)):
        u = rng.normal(0.0, 1.0, 2)
        p, v, f, _ = draw(rng, 1, rows, 0.05, 0.02, u, BATCH_DT, frames)
        add(name, p, v, f, u)
    u = rng.normal(0.0, 1.0, 2)
    p, v, f, _ = draw(rng, 1, 24, 0.05, 0.02, u, BATCH_DT)
    v[7, 0] = 0.0
    add("directed, one zero variance", p, v, f, u)
    return {"pos": np.ascontiguousarray(np.concatenate([pos] + [q[0] for q in parts])),
            "var": np.ascontiguousarray(np.concatenate([b["var"]] + [q[1] for q in parts])),
            "frames": np.concatenate([b["frames"]] + [q[2] for q in parts]).astype(np.int32),
            "use": np.concatenate([b["use"]] + [q[3] for q in parts]),
            "offsets": np.concatenate([b["offsets"], b["offsets"][-1] + np.cumsum([len(q[0]) for q in parts])]).astype(np.int64),
            "names": b["names"] + names, "D": np.array(Ds), "velocity": np.ascontiguousarray(np.array(vels))}
