"""Shared by tests/test_localize2.py and tests/test_localize2_gpu.py: the two-emitter image model written from its definition,
an independent Fisher matrix by central differences, the read-only case tables of the joint fit (csrc/localize2.hip,
helpers/tracking._fit_mle2_numpy), the neighbour tables and the bars, with their origin.

Parameters are (N1, x1, y1, N2, x2, y2, s, b) throughout.

The bars
  exact_tolerance: the fit of an expected image rounded to float32.  The rounding moves pixel t by delta_t with |delta_t| <=
  2^-24 mu_t; to first order the estimate moves by F^-1 sum_t J_t delta_t / mu_t, and by Cauchy-Schwarz its k-th entry by at
  most sqrt((F^-1)_kk) sqrt(sum_t delta_t^2 / mu_t) <= 2^-24 sqrt(CRLB_k sum_t mu_t), with the CRLB from fisher_fd at the
  planted parameters.  A factor 2 for the higher orders, plus the stopping rule's own 1e-11 of the parameter's scale.  (test_localize.py
  has no such check for one emitter to take a tolerance from.)
  FD_STEP = 1e-5 and FD_RTOL = 1e-6: a central difference of step h has a truncation error of h^2 / 6 f''' / f' ~ 2e-11 for
  scales of one pixel and a rounding error of eps |mu| / (h |dmu|) ~ 1e-16 * 1e3 / 1e-5 = 1e-8 per pixel at worst, which averages over
  the pixels; inverting the 8 x 8 matrix (condition number up to ~1e7 in (N, x, y, s, b) units, far less after the scaling by
  its diagonal that the comparison applies) leaves the diagonal of the inverse within 1e-6 relative.
  KERNEL_FIT_RTOL (tracking_common) for kernel against restatement, as tests/test_localize_gpu.py.
  The statistical bar of the issue: m = 4 / sqrt(2 n) plus the excess of the single-emitter fit on isolated spots."""
import functools
import math

import numpy as np

import localize_common as LC

FD_STEP, FD_RTOL = 1e-5, 1e-6


def model(P, p, count=2, read_var=0.0):
    """mu [n, P, P] at p [n, 8] (fp64), from the definition; count 1 drops emitter 2."""
    p = np.atleast_2d(np.asarray(p, dtype=np.float64))
    out = np.empty((len(p), P, P))
    for i, q in enumerate(p):
        mu = q[7] + q[0] * LC.pixel_integral(P, q[2:3], q[6])[0][:, None] * LC.pixel_integral(P, q[1:2], q[6])[0][None, :]
        if count == 2:
            mu = mu + q[3] * LC.pixel_integral(P, q[5:6], q[6])[0][:, None] * LC.pixel_integral(P, q[4:5], q[6])[0][None, :]
        out[i] = mu + read_var
    return out


def fisher_fd(P, p, free, count=2, read_var=0.0):
    """Fisher matrix [k, k] of the free parameters at p [8]: dmu/dp by central differences of step FD_STEP (relative to the
    parameter for photons and background, absolute in pixels otherwise), sum dmu dmu^T / mu."""
    p = np.asarray(p, dtype=np.float64)
    mu = model(P, p, count, read_var)[0]
    dmu = []
    for k in free:
        h = FD_STEP * (abs(p[k]) if k in (0, 3, 7) else 1.0)
        hi, lo = p.copy(), p.copy()
        hi[k] += h
        lo[k] -= h
        dmu.append((model(P, hi, count, read_var)[0] - model(P, lo, count, read_var)[0]) / (hi[k] - lo[k]))
    dmu = np.stack(dmu).reshape(len(free), -1)
    return (dmu / mu.reshape(1, -1)) @ dmu.T


def bound_fd(P, p, free, count=2, read_var=0.0):
    """diagonal of the inverse of fisher_fd, inverted after scaling by its diagonal"""
    F = fisher_fd(P, p, free, count, read_var)
    s = 1.0 / np.sqrt(np.diag(F))
    return np.diag(np.linalg.inv(F * s[:, None] * s[None, :])) * s * s


def exact_tolerance(P, truth, free):
    """per free parameter: 2 * 2^-24 sqrt(CRLB_k sum(mu)) + 1e-11 max(|truth_k|, 1) (module docstring)"""
    truth = np.asarray(truth, dtype=np.float64)
    total = float(model(P, truth).sum())
    return 2.0 * 2.0 ** -24 * np.sqrt(bound_fd(P, truth, free) * total) + 1e-11 * np.maximum(np.abs(truth[free]), 1.0)


def free_parameters(count, fit_sigma):
    free = [0, 1, 2] + ([3, 4, 5] if count == 2 else []) + ([6] if fit_sigma else []) + [7]
    return free


# ----------------------------------------------------------------------------------------------------------------------
# exact images: (P, separation, angle in degrees, N1, N2, sigma, background)
# ----------------------------------------------------------------------------------------------------------------------
EXACT = [(P, sep, ang, n1, n2, s, 8.0)
         for P, s, seps in ((7, 1.0, (2.5, 3.0)), (9, 1.3, (2.5, 4.0)), (15, 1.6, (3.5, 6.0)))
         for sep in seps for ang in (0.0, 37.0, 90.0, 200.0) for n1, n2 in ((1000.0, 1000.0), (500.0, 2000.0))]


def exact_case(case):
    """-> (patch [1, P, P] float32, truth [8], guess [1, 4]): the primary 0.2 / -0.3 px off the centre, the guesses at the
    nearest integers"""
    P, sep, ang, n1, n2, s, b = case
    x1, y1 = P // 2 + 0.2, P // 2 - 0.3
    x2, y2 = x1 + sep * math.cos(math.radians(ang)), y1 + sep * math.sin(math.radians(ang))
    truth = np.array([n1, x1, y1, n2, x2, y2, s, b])
    guess = np.array([[float(P // 2), float(P // 2), float(np.rint(x2)), float(np.rint(y2))]])
    return model(P, truth).astype(np.float32), truth, guess


# ----------------------------------------------------------------------------------------------------------------------
# Poisson tables for kernel against restatement: name -> (P, sigma, fit_sigma, gain, offset, read_var, seed)
# ----------------------------------------------------------------------------------------------------------------------
TABLE_N = 257
CASES = {
    "p5_fixed": (5, 0.6, False, 1.0, 0.0, 0.0, 31),
    "p9": (9, 1.3, True, 1.0, 0.0, 0.0, 32),
    "p9_fixed_camera": (9, 1.3, False, 0.5, 20.0, 0.0, 33),
    "p15_camera": (15, 1.8, True, 1.7, 50.0, 1.0, 34),
}
SIZES = (1, 63, 64, 65, 257)          # the lane group is a wave: 63, 64 and 65 are its edges too


def camera_kwargs(name):
    P, sigma, fs, gain, offset, read_var, _ = CASES[name]
    return {"gain": gain, "offset": offset, "read_var": read_var, "sigma0": sigma, "fit_sigma": fs}


@functools.lru_cache(maxsize=None)
def case_table(name):
    """(patches [TABLE_N, P, P] float32, count [TABLE_N] int32, guess [TABLE_N, 4]), read-only.  Every third row has one
    emitter, the others a pair min(0.4 P, P / 2 - 0.9) apart at a random angle, 1000 and 600 photons on a background of 10; rows 5, 6 and 7 are
    built to fail: an empty patch, a pair whose guesses coincide on one true emitter, a single spot fitted as two with both
    guesses on it (coincident guesses are a singular start)."""
    P, sigma, _, gain, offset, read_var, seed = CASES[name]
    rng = np.random.default_rng(seed)
    n = TABLE_N
    count = np.where(np.arange(n) % 3 == 2, 1, 2).astype(np.int32)
    x1, y1 = P // 2 + rng.uniform(-0.5, 0.5, (2, n))
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    sep = min(0.4 * P, P / 2 - 0.9)                                       # the neighbour's centre stays inside the patch
    x2, y2 = x1 + sep * np.cos(ang), y1 + sep * np.sin(ang)
    truth = np.stack([np.full(n, 1000.0), x1, y1, np.full(n, 600.0), x2, y2, np.full(n, sigma), np.full(n, 10.0)], axis=1)
    count[[5, 6]] = 2
    count[7] = 2
    mu = np.where((count == 2)[:, None, None], model(P, truth, 2), model(P, truth, 1))
    if read_var == 0:
        mu[5] = 0.0
    mu[7] = model(P, truth[7:8], 1)[0]
    e = rng.poisson(mu).astype(np.float64)
    if read_var > 0:
        e = e + rng.normal(0.0, math.sqrt(read_var), e.shape)
    patches = (offset + gain * e).astype(np.float32)
    if read_var == 0:
        patches[5] = offset                                                # no photon at all (with a readout variance the data are never 0)
    guess = np.stack([np.full(n, float(P // 2)), np.full(n, float(P // 2)), np.rint(x2), np.rint(y2)], axis=1)
    guess[6, 2:] = guess[6, :2]
    guess[7, 2:] = guess[7, :2]
    for a in (patches, count, guess):
        a.setflags(write=False)
    return patches, count, guess


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The host restatement on the whole table of a case, computed once: (params, crlb, deviance, status, iterations)."""
    from moleculardiffusion_mivit_amd.helpers import tracking as T
    out = T._fit_mle2_numpy(*case_table(name), **camera_kwargs(name))
    for a in out:
        a.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# statistics (the issue's inputs)
# ----------------------------------------------------------------------------------------------------------------------
STAT = {"n": 2000, "seed": 41, "P": 9, "sigma": 1.3, "photons": 1000.0, "background": 10.0, "separation": 4.0}


def stat_margin(n):
    return 4.0 / math.sqrt(2.0 * n)


@functools.lru_cache(maxsize=None)
def stat_pairs():
    """(patches, truth [n, 8], guess [n, 4]) of the Poisson pairs, and (patches, cx, cy) of isolated spots of the same
    brightness drawn after them."""
    n, P, s, N, b, sep = (STAT[k] for k in ("n", "P", "sigma", "photons", "background", "separation"))
    rng = np.random.default_rng(STAT["seed"])
    x1, y1 = P // 2 + rng.uniform(-0.5, 0.5, (2, n))
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    x2, y2 = x1 + sep * np.cos(ang), y1 + sep * np.sin(ang)
    truth = np.stack([np.full(n, N), x1, y1, np.full(n, N), x2, y2, np.full(n, s), np.full(n, b)], axis=1)
    patches = rng.poisson(model(P, truth)).astype(np.float32)
    guess = np.stack([np.full(n, float(P // 2)), np.full(n, float(P // 2)), np.rint(x2), np.rint(y2)], axis=1)
    cx, cy = P // 2 + rng.uniform(-0.5, 0.5, (2, n))
    alone = rng.poisson(LC.expected_image(P, N, b, s, cx, cy)).astype(np.float32)
    return (patches, truth, guess), (alone, cx, cy)


def mean_true_bound(P, truth, count, every=10):
    """mean over every `every`-th row of the bound at the true parameters (fisher_fd) -> (x, y) of the primary"""
    free = free_parameters(count, True)
    v = np.array([bound_fd(P, t, free, count) for t in truth[::every]])
    return float(v[:, 1].mean()), float(v[:, 2].mean())


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


# ----------------------------------------------------------------------------------------------------------------------
# neighbour tables: (frames, ys, xs, reach)
# ----------------------------------------------------------------------------------------------------------------------
def neighbour_tables():
    rng = np.random.default_rng(51)
    dense = (rng.integers(0, 6, 300), rng.integers(0, 24, 300), rng.integers(0, 24, 300))
    out = {
        "empty": (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 3),
        "one_row": (np.array([2]), np.array([5]), np.array([7]), 3),
        "empty_frames_between": (np.array([0, 0, 4, 4, 9]), np.array([5, 7, 5, 20, 1]), np.array([5, 6, 5, 5, 1]), 3),
        # row 0 has rows 1 .. 4 at the same distance (ties to the lower row), row 5 sits on row 6 (distance 0)
        "ties": (np.zeros(7, np.int64), np.array([10, 8, 12, 10, 10, 30, 30]), np.array([10, 10, 10, 8, 12, 30, 30]), 2),
        "reach_0": (np.zeros(4, np.int64), np.array([3, 3, 4, 9]), np.array([3, 3, 3, 9]), 0),
        "unsorted": (np.array([3, 1, 3, 0, 1, 3, 1]), np.array([5, 5, 6, 5, 7, 9, 30]), np.array([5, 5, 7, 5, 5, 5, 30]), 4),
        "dense_unsorted": dense + (4,),
        "dense_reach_1": dense + (1,),
    }
    return out


def brute_neighbours(frames, ys, xs, reach):
    n = len(frames)
    nb, cnt = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        best = None
        for j in range(n):
            if j == i or frames[j] != frames[i]:
                continue
            dy, dx = abs(int(ys[j]) - int(ys[i])), abs(int(xs[j]) - int(xs[i]))
            if max(dy, dx) > reach:
                continue
            cnt[i] += 1
            d2 = dy * dy + dx * dx
            if best is None or d2 < best:
                best, nb[i] = d2, j
    return nb, cnt


# ----------------------------------------------------------------------------------------------------------------------
# end to end: two slow particles about 4.5 px apart, the Poisson camera of DESIGN 4o
# ----------------------------------------------------------------------------------------------------------------------
SCENE = {"F": 20, "H": 48, "W": 48, "P": 11, "seed": 2, "separation": 4.5, "step": 0.05, "peak": 150.0, "sigma": 1.3,
         "camera": {"background": 10.0, "gain": 2.0, "offset": 100.0}}


@functools.lru_cache(maxsize=None)
def scene():
    """(movie [F, H, W] float32 numpy in camera units, truth positions [2, F, 2] (y, x), sigma in pixels, photons per spot):
    generation.render_movie (PSF width SCENE["sigma"] px) of two particles that start SCENE["separation"] apart and take Gaussian steps of SCENE["step"] px
    per frame and axis, then Poisson(image + background) * gain + offset, all drawn from numpy's generator on the host."""
    import torch
    from moleculardiffusion_mivit_amd.helpers import generation as G
    props = dict(G.DEFAULT_IMAGE_PROPS)
    up = props["upsampling_factor"]
    sigma_hr = SCENE["sigma"] * up              # narrower than the default optics: the detector must resolve the pair
    rng = np.random.default_rng(SCENE["seed"])
    F, H, W = SCENE["F"], SCENE["H"], SCENE["W"]
    ang = math.radians(30.0)
    start = np.array([[24.2, 21.8], [24.2 + SCENE["separation"] * math.sin(ang), 21.8 + SCENE["separation"] * math.cos(ang)]])
    pos = start[:, None, :] + np.cumsum(rng.normal(0.0, SCENE["step"], (2, F, 2)), axis=1)
    amp = np.full((2, F, 1), SCENE["peak"])
    clean = G.render_movie(torch.from_numpy(pos), torch.from_numpy(amp), sigma_hr, H, W, up).numpy()
    cam = SCENE["camera"]
    movie = (cam["offset"] + cam["gain"] * rng.poisson(clean + cam["background"])).astype(np.float32)
    sigma = sigma_hr / up
    movie.setflags(write=False)
    return movie, pos, sigma, SCENE["peak"] * 2.0 * math.pi * sigma * sigma


def scene_pipeline(movie):
    """detect -> patches -> refine with and without neighbours, on the device the movie lives on (numpy: the host) ->
    (frames, iy, ix, single, joint) with the two result dicts as numpy arrays"""
    import torch
    from moleculardiffusion_mivit_amd.helpers import tracking as T
    _, _, sigma, _ = scene()
    camera = {"gain": SCENE["camera"]["gain"], "offset": SCENE["camera"]["offset"], "sigma0": sigma}
    coords, _ = T.detect_particles_movie(movie, return_dog=False)
    frames = np.concatenate([np.full(len(c), f) for f, c in enumerate(coords)])
    iy, ix = np.concatenate([c[:, 0] for c in coords]), np.concatenate([c[:, 1] for c in coords])
    patches = T.extract_patches_flat(movie, frames, iy, ix, SCENE["P"])
    if torch.is_tensor(movie):
        fr, yy, xx = (torch.from_numpy(a).to(movie.device) for a in (frames, iy, ix))
        single = T.refine_localizations_tensors(patches, yy, xx, method="mle", camera=camera)
        joint = T.refine_localizations_tensors(patches, yy, xx, method="mle", camera=camera, frames=fr, neighbours=True)
        single, joint = ({k: v.cpu().numpy() for k, v in r.items()} for r in (single, joint))
    else:
        single = T.refine_localizations(patches, iy, ix, method="mle", camera=camera)
        joint = T.refine_localizations(patches, iy, ix, method="mle", camera=camera, frames=frames, neighbours=True)
    return frames, iy, ix, single, joint


def scene_errors(frames, iy, ix, res):
    """every detection matched to the nearer planted particle of its frame -> (errors y, errors x) of the refined positions"""
    _, pos, _, _ = scene()
    truth = pos[:, frames, :]                                                             # [2, N, 2]
    which = np.argmin(np.hypot(truth[:, :, 0] - iy, truth[:, :, 1] - ix), axis=0)
    rows = np.arange(len(frames))
    return res["y_refined"] - truth[which, rows, 0], res["x_refined"] - truth[which, rows, 1]


def scene_bound():
    """mean over the frames of the bound at the planted parameters for either particle as the primary of a P x P patch centred
    on its rounded position -> (y, x) variances"""
    _, pos, sigma, photons = scene()
    P, half = SCENE["P"], SCENE["P"] // 2
    vy, vx = [], []
    for f in range(SCENE["F"]):
        for a in (0, 1):
            oy, ox = np.rint(pos[a, f, 0]) - half, np.rint(pos[a, f, 1]) - half
            p = [photons, pos[a, f, 1] - ox, pos[a, f, 0] - oy, photons, pos[1 - a, f, 1] - ox, pos[1 - a, f, 0] - oy, sigma,
                 SCENE["camera"]["background"]]
            v = bound_fd(P, p, free_parameters(2, True))
            vy.append(v[2]), vx.append(v[1])
    return float(np.mean(vy)), float(np.mean(vx))
