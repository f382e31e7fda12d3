"""Real-data patch extraction (reference helpers/helpersTracking.py:513-550 ``extract_particle_patches``): square patches around
every tracked position, zero-padded at the image border -- the tensors a trained MiViT consumes on experimental movies
(SURVEY section 8 row f4).  One gather for all positions of a track; works on CPU or GPU tensors.

The rest of the reference's real-movie front end (helpers/helpersTracking.py) is here too: detect_particles (:12-57),
link_particles (:123-178), track_particles (:180-336), analyze_microscopy_sequence (:436-510),
add_refined_localization_to_dataframe (:555-604), compute_displacement (:608-647), tracks_to_dataframe (:653-681).  A CUDA
movie goes to the kernels of csrc/tracking.hip (detection for the whole movie at once, one Gaussian fit per patch) and what
the reference returns as images stays a CUDA tensor; anything else goes to the numpy restatement in this file, which computes
the filter in the kernel's order (bitwise equal) and the fit with the kernel's algorithm.  Linking is a Hungarian assignment
per frame pair: by default (linking="host") scipy's, in a loop over the frames on the host, as the reference does it; with
linking="device" all frame pairs of a movie are solved in one launch of csrc/linking.hip and the track ids are chained on the
device (link_particles_movie, chain_tracks, track_particles_tensors); with max_gap > 0 the end of a track is then linked to the
start of a later one across up to max_gap missed frames (close_gaps_movie) and the missed frames become rows with an
interpolated position (fill_gaps), so that every track stays contiguous in frames.  Beside the reference's detector stands a
likelihood-ratio detector on the photon-counting camera model with a per-pixel false-alarm probability
(detect_particles_lrt_movie, csrc/detect.hip; detector={"method": "lrt", ...} on the tracking functions).  Movies are filtered as float32.  pandas and scipy are only
imported by the functions that need them: detect_particles_movie, track_particles_flat, extract_patches_flat and
refine_localizations need neither pandas nor (except for linking) scipy."""
import math
from typing import Dict, Sequence, Tuple

import numpy as np
import torch


def extract_particle_patches(image_3d, tracks: Dict[object, Sequence[Tuple[int, float, float]]], patch_size: int = 7):
    """image_3d (num_frames, H, W) array / tensor; tracks {id: [(frame, y, x), ...]} -> {id: (len, patch, patch)} of the input's
    kind (numpy in, numpy out).  Positions are rounded to the nearest pixel; pixels outside the image read as 0."""
    assert patch_size % 2 == 1, "patch_size must be an odd number"
    is_np = not torch.is_tensor(image_3d)
    img = torch.as_tensor(np.asarray(image_3d)) if is_np else image_3d
    half = patch_size // 2
    nf, H, W = img.shape
    off = torch.arange(-half, half + 1, device=img.device)
    out = {}
    for tid, positions in tracks.items():
        if len(positions) == 0:
            out[tid] = np.array([]) if is_np else img.new_zeros((0, patch_size, patch_size))
            continue
        pos = np.asarray(positions, dtype=np.float64)
        fr = torch.as_tensor(pos[:, 0].astype(np.int64), device=img.device)
        # Python's round() (round-half-to-even), like the reference's int(round(y))
        yy = torch.as_tensor(np.rint(pos[:, 1]).astype(np.int64), device=img.device)
        xx = torch.as_tensor(np.rint(pos[:, 2]).astype(np.int64), device=img.device)
        ys = yy[:, None] + off[None, :]                       # (L, p)
        xs = xx[:, None] + off[None, :]
        ok = ((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :]
        g = img[fr[:, None, None], ys.clamp(0, H - 1)[:, :, None], xs.clamp(0, W - 1)[:, None, :]]
        g = torch.where(ok, g, torch.zeros((), dtype=img.dtype, device=img.device))
        out[tid] = g.numpy() if is_np else g
    return out


# ----------------------------------------------------------------------------------------------------------------------
# detection
# ----------------------------------------------------------------------------------------------------------------------
FIT_XTOL = 1e-11          # every parameter's undamped step relative to its scale (MINPACK's default would be 1.49e-8)
FIT_MAX_ITER = 100
FIT_COST_SLACK = 1.0 + 1e-13
FALLBACK_PSF_SIZE = 10    # the reference's psf_size for a patch whose fit failed


def gaussian_half_kernel(sigma, truncate=4.0):
    """The weights scipy.ndimage.gaussian_filter uses (scipy.ndimage._filters._gaussian_kernel1d, order 0), centre first:
    w[0] the centre, w[k] the weight at distance k, radius int(truncate * sigma + 0.5)."""
    sd = float(sigma)
    if not sd > 0:
        raise ValueError(f"sigma must be positive, got {sigma}")
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def _is_cuda(x):
    return torch.is_tensor(x) and x.device.type == "cuda"


def _correlate_axis(x32, w, axis):
    """scipy.ndimage.correlate1d of a float32 [F, H, W] array along one axis with a symmetric kernel, mode 'reflect': fp64 sum
    in scipy's order (centre, then the outermost pair inwards), rounded to float32."""
    r = len(w) - 1
    n = x32.shape[axis]
    pad = [(0, 0)] * 3
    pad[axis] = (r, r)
    xp = np.pad(x32, pad, mode="symmetric").astype(np.float64)

    def at(o):
        idx = [slice(None)] * 3
        idx[axis] = slice(r + o, r + o + n)
        return xp[tuple(idx)]

    acc = at(0) * w[0]
    for k in range(r, 0, -1):
        acc = acc + (at(-k) + at(k)) * w[k]
    return acc.astype(np.float32)


def _dog_numpy(movie32, w1, w2, chunk=16):
    """gaussian_filter(frame, sigma1) - gaussian_filter(frame, sigma2) of every float32 frame, in the kernel's order."""
    out = np.empty(movie32.shape, np.float32)
    for f0 in range(0, movie32.shape[0], chunk):
        x = movie32[f0:f0 + chunk]
        g1 = _correlate_axis(_correlate_axis(x, w1, 1), w1, 2)
        g2 = _correlate_axis(_correlate_axis(x, w2, 1), w2, 2)
        out[f0:f0 + chunk] = (g1 - g2) + np.float32(0.0)          # + 0: -0.0 and +0.0 are one value, as in the kernel
    return out


def _window_max(frame, m):
    """Maximum over the (2 m + 1) square window with replicated borders (scipy.ndimage.maximum_filter, mode 'nearest')."""
    H, W = frame.shape
    p = np.pad(frame, ((m, m), (0, 0)), mode="edge")
    v = p[0:H]
    for k in range(1, 2 * m + 1):
        v = np.maximum(v, p[k:k + H])
    p = np.pad(v, ((0, 0), (m, m)), mode="edge")
    v = p[:, 0:W]
    for k in range(1, 2 * m + 1):
        v = np.maximum(v, p[:, k:k + W])
    return v


def _peaks_numpy(dog, threshold_percentage, min_distance, absolute=None):
    """peak_local_max(dog, min_distance, threshold_abs=threshold_percentage * dog.max(), exclude_border=False) of one float32
    frame -> (coords [n, 2] int64 (y, x), number of candidates before spacing).  absolute: a float32 threshold that takes the
    place of threshold_percentage * dog.max() (the likelihood-ratio detector)."""
    if absolute is not None:
        thr = np.float32(absolute)
    else:
        thr = np.float32(threshold_percentage) * dog.max()         # one float32 product, as numpy 2 does it
    mask = dog == _window_max(dog, min_distance)
    if mask.all():                                                 # a flat frame has no peak
        return np.zeros((0, 2), np.int64), 0
    mask &= dog > thr
    ys, xs = np.nonzero(mask)                                      # row-major
    order = np.argsort(-dog[ys, xs], kind="stable")                # value descending, ties by row-major index
    ys, xs = ys[order], xs[order]
    ky, kx = np.empty(len(ys), np.int64), np.empty(len(ys), np.int64)
    n = 0
    for y, x in zip(ys, xs):
        if n == 0 or not np.any((np.abs(ky[:n] - y) <= min_distance) & (np.abs(kx[:n] - x) <= min_distance)):
            ky[n], kx[n] = y, x
            n += 1
    return np.stack([ky[:n], kx[:n]], axis=1), len(ys)


def _check_detection_args(shape, sigma1, sigma2, min_distance):
    if len(shape) != 3:
        raise ValueError(f"movie must be [F, H, W], got {tuple(shape)}")
    if not (0 < float(sigma1) <= float(sigma2)):
        raise ValueError(f"need 0 < sigma1 <= sigma2, got {sigma1}, {sigma2}")
    if int(min_distance) != min_distance or not 1 <= min_distance <= 16:
        raise ValueError(f"min_distance must be an integer from 1 to 16, got {min_distance}")
    w1, w2 = gaussian_half_kernel(sigma1), gaussian_half_kernel(sigma2)
    r2 = len(w2) - 1
    if r2 > 16:
        raise ValueError(f"sigma2 = {sigma2} gives a filter radius of {r2} > 16")
    if shape[1] <= r2 or shape[2] <= r2:
        raise ValueError(f"frames of {shape[1]} x {shape[2]} are not larger than the filter radius {r2} of sigma2 = {sigma2}")
    return w1, w2


def detect_particles_movie(movie, sigma1=1.0, sigma2=2.0, threshold_percentage=0.1, min_distance=3,
                           max_peaks_per_frame=512, return_dog=True):
    """detect_particles of every frame of a movie [F, H, W] at once -> (list of F coordinate arrays [n_f, 2] int64 (y, x),
    strongest first, and the DoG movie [F, H, W] float32 of the input's kind, or None with return_dog=False).  A CUDA tensor
    runs on the GPU (ops.dog_peaks) and raises if a frame has more than max_peaks_per_frame candidates."""
    w1, w2 = _check_detection_args(movie.shape, sigma1, sigma2, min_distance)
    if _is_cuda(movie):
        from .. import ops
        count, coords, _, dog = ops.dog_peaks(movie.float(), w1, w2, threshold_percentage, int(min_distance),
                                              max_peaks_per_frame, return_dog)
        count = count.cpu().numpy()
        top = int(count.max()) if len(count) else 0
        coords = coords[:, :top].cpu().numpy().astype(np.int64)
        return [coords[f, :count[f]] for f in range(len(count))], dog
    was_tensor = torch.is_tensor(movie)
    arr = np.ascontiguousarray(movie.detach().numpy() if was_tensor else np.asarray(movie), dtype=np.float32)
    dog = _dog_numpy(arr, w1, w2)
    coords = [_peaks_numpy(dog[f], threshold_percentage, int(min_distance))[0] for f in range(len(dog))]
    if not return_dog:
        return coords, None
    return coords, (torch.from_numpy(dog) if was_tensor else dog)


def detect_particles(image, sigma1=1.0, sigma2=2.0, threshold_percentage=0.1, min_distance=3):
    """Reference detect_particles: one frame [H, W] -> (coordinates [n, 2] (y, x), dog_image)."""
    if len(image.shape) != 2:
        raise ValueError(f"image must be [H, W], got {tuple(image.shape)}; use detect_particles_movie for a movie")
    coords, dog = detect_particles_movie(image[None], sigma1, sigma2, threshold_percentage, min_distance)
    return coords[0], dog[0]


# ----------------------------------------------------------------------------------------------------------------------
# likelihood-ratio detection on the photon-counting camera (csrc/detect.hip)
# ----------------------------------------------------------------------------------------------------------------------
LRT_MAX_RADIUS = 7
LRT_MAX_PEAKS = 2048
_DETECTOR_DEFAULTS = {"gain": 1.0, "offset": 0.0, "read_var": 0.0, "sigma0": 1.0, "radius": None, "p_fa": 1e-6}


def detection_threshold(p_fa):
    """The threshold t = z^2, z = -Phi^-1(p_fa), at which a statistic whose square root is a one-sided standard normal under
    "background only" is exceeded with probability p_fa per pixel; 0 < p_fa <= 0.5."""
    from statistics import NormalDist
    p = float(p_fa)
    if not 0.0 < p <= 0.5:
        raise ValueError(f"p_fa must lie in (0, 0.5], got {p_fa}")
    z = -NormalDist().inv_cdf(p)
    return z * z


def psf_profile(sigma0, radius=None):
    """The pixel-integrated Gaussian of fit_spots_mle centred on a pixel centre: e[i + r] = 1/2 [erf((i + 1/2) / (sqrt(2)
    sigma0)) - erf((i - 1/2) / (sqrt(2) sigma0))] for i = -r .. r, float64 [2 r + 1]; r = radius, by default ceil(3 sigma0),
    from 1 to LRT_MAX_RADIUS."""
    s = float(sigma0)
    if not (s > 0 and math.isfinite(s)):
        raise ValueError(f"sigma0 must be finite and > 0, got {sigma0}")
    r = math.ceil(3.0 * s) if radius is None else radius
    if int(r) != r or not 1 <= r <= LRT_MAX_RADIUS:
        raise ValueError(f"radius must be an integer from 1 to {LRT_MAX_RADIUS}, got {r}"
                         + (f" = ceil(3 sigma0) for sigma0 = {sigma0}" if radius is None else ""))
    r = int(r)
    w = _SQRT2 * s
    e = np.array([0.5 * (math.erf((i + 0.5) / w) - math.erf((i - 0.5) / w)) for i in range(-r, r + 1)], dtype=np.float64)
    if not e.min() > 0.0:
        raise ValueError(f"sigma0 = {sigma0} is too small for a radius of {r}: the profile vanishes at its ends")
    return e


def _lrt_axis(n_pix, e):
    """Count, sum e and sum e^2 over the offsets of the clipped window of every index of one axis, in ascending order."""
    r = len(e) // 2
    idx = np.arange(n_pix)
    n, g, q = np.zeros(n_pix), np.zeros(n_pix), np.zeros(n_pix)
    for k in range(-r, r + 1):
        valid = (idx + k >= 0) & (idx + k < n_pix)
        n = n + valid
        g = g + np.where(valid, e[k + r], 0.0)
        q = q + np.where(valid, e[k + r] * e[k + r], 0.0)
    return n, g, q


def _score_numpy(movie32, e, gain=1.0, offset=0.0, read_var=0.0, chunk=16, dtype=np.float32):
    """The score map of csrc/detect.hip::sc_map_kernel for a float32 movie [F, H, W], bitwise: S = U^2 / V where U, V > 0
    and 0 elsewhere, float32 (dtype=np.float64: the statistic before that rounding).  Windows are clipped at the frame edge;
    a pixel outside the frame enters a sum as + 0.0, which leaves every bit of it, so the passes run over a zero-padded
    copy."""
    F, H, W = movie32.shape
    r = len(e) // 2
    ny, gy, qy = _lrt_axis(H, e)
    nx, gx, qx = _lrt_axis(W, e)
    n, Sg, Sgg = ny[:, None] * nx[None, :], gy[:, None] * gx[None, :], qy[:, None] * qx[None, :]
    out = np.empty(movie32.shape, dtype)
    for f0 in range(0, F, chunk):
        d = _mle_data(movie32[f0:f0 + chunk], gain, offset, read_var)
        dp = np.pad(d, ((0, 0), (r, r), (0, 0)))
        A, B = np.zeros(d.shape), np.zeros(d.shape)
        for k in range(2 * r + 1):                                # ascending dy
            v = dp[:, k:k + H, :]
            A = A + e[k] * v
            B = B + v
        Ap, Bp = np.pad(A, ((0, 0), (0, 0), (r, r))), np.pad(B, ((0, 0), (0, 0), (r, r)))
        Sgd, Sd = np.zeros(d.shape), np.zeros(d.shape)
        for k in range(2 * r + 1):                                # ascending dx
            Sgd = Sgd + e[k] * Ap[:, :, k:k + W]
            Sd = Sd + Bp[:, :, k:k + W]
        with np.errstate(all="ignore"):
            mu0 = Sd / n
            U = Sgd - mu0 * Sg
            V = mu0 * (Sgg - Sg * Sg / n)
            ok = (U > 0.0) & (V > 0.0)
            out[f0:f0 + chunk] = np.where(ok, U * U / np.where(ok, V, 1.0), 0.0).astype(dtype)
    return out


def _lrt_solve(n, lam):
    """(A + lam diag(A)) step = -g of the 2 x 2 system by Cholesky (csrc/spot_fit.h::sf_solve<2>) -> (d_theta, d_beta, ok)."""
    with np.errstate(all="ignore"):
        s = n["a00"] + lam * n["a00"]
        ok = (s > 0.0) & (s < 1e300)
        L00 = np.sqrt(np.where(ok, s, 1.0))
        L10 = n["a10"] / L00
        s = n["a11"] + lam * n["a11"]
        s = s - L10 * L10
        ok &= (s > 0.0) & (s < 1e300)
        L11 = np.sqrt(np.where(ok, s, 1.0))
        z0 = -n["g0"] / L00
        z1 = (-n["g1"] - L10 * z0) / L11
        d1 = z1 / L11
        d0 = (z0 - L10 * d1) / L00
    return d0, d1, ok


def _lrt_eval(d, g, valid, theta, beta):
    """lr_eval: deviance, 2 sum(mu + d), gradient, Fisher matrix and the out-of-domain flag of mu = theta g + beta for windows
    d / g / valid [n, K] flattened row-major; a pixel outside the frame adds + 0.0 to every sum."""
    n = len(theta)
    acc = {k: np.zeros(n) for k in ("cost", "mag", "g0", "g1", "a00", "a10", "a11")}
    whole = bool(valid.all())
    with np.errstate(all="ignore"):
        bad = ~(theta > 0.0)
        for t in range(d.shape[1]):
            ok = valid[:, t]
            if not whole and not ok.any():
                continue
            m = (lambda v: v) if whole else (lambda v: np.where(ok, v, 0.0))
            gt, dd = g[:, t], d[:, t]
            mu = theta * gt + beta
            bad |= ok & ~(mu > 0.0)
            rm = 1.0 / mu
            r = dd * rm
            pos = dd > 0.0
            acc["cost"] = acc["cost"] + m(np.where(pos, (mu - dd) + dd * np.log(np.where(pos, r, 1.0)), mu))
            acc["mag"] = acc["mag"] + m(mu + dd)
            w = 1.0 - r
            acc["g0"] = acc["g0"] + m(gt * w)
            acc["g1"] = acc["g1"] + m(w)
            gr = gt * rm
            acc["a00"] = acc["a00"] + m(gr * gt)
            acc["a10"] = acc["a10"] + m(rm * gt)
            acc["a11"] = acc["a11"] + m(rm)
        acc["cost"], acc["mag"] = 2.0 * acc["cost"], 2.0 * acc["mag"]
    acc["bad"] = bad
    return acc


def _lrt_numpy(movie32, e, gain, offset, read_var, frames, ys, xs, xtol=FIT_XTOL, max_iter=FIT_MAX_ITER, chunk=1 << 16):
    """The likelihood ratio of csrc/detect.hip::lr_fit at the pixels (frames, ys, xs) [n] of a float32 movie [F, H, W], all of
    them side by side -> (T [n], theta [n], beta [n] float64, status [n] int32).  mu = theta g + beta over the clipped window,
    every sum in window row-major order; equal to the kernel apart from log.  Start: the least-squares point theta = U / den,
    beta = mu0 - theta Sg / n; where that beta is not positive, beta = mu0 / 1000 and theta = (Sd - n beta) / Sg, which keeps
    the window's total.  A pixel whose U, den or mu0 is not positive has its maximum at theta = 0: T = 0, beta = mu0."""
    frames, ys, xs = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (frames, ys, xs))
    N = len(frames)
    if N > chunk:
        parts = [_lrt_numpy(movie32, e, gain, offset, read_var, frames[a:a + chunk], ys[a:a + chunk], xs[a:a + chunk], xtol,
                            max_iter, chunk) for a in range(0, N, chunk)]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
    T, theta, beta, status = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N, np.int32)
    if N == 0:
        return T, theta, beta, status
    _, H, W = movie32.shape
    r = len(e) // 2
    K = 2 * r + 1
    off = np.arange(-r, r + 1)
    yy, xx = ys[:, None] + off, xs[:, None] + off
    valid = (((yy >= 0) & (yy < H))[:, :, None] & ((xx >= 0) & (xx < W))[:, None, :]).reshape(N, K * K)
    raw = movie32[frames[:, None, None], np.clip(yy, 0, H - 1)[:, :, None], np.clip(xx, 0, W - 1)[:, None, :]]
    d = np.where(valid, _mle_data(raw, gain, offset, read_var).reshape(N, K * K), 0.0)
    g = np.where(valid, (e[:, None] * e[None, :]).reshape(1, K * K), 0.0)
    n, Sd, Sgd, Sg, Sgg = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    for t in range(K * K):
        n = n + valid[:, t]
        Sd = Sd + d[:, t]
        Sgd = Sgd + g[:, t] * d[:, t]
        Sg = Sg + g[:, t]
        Sgg = Sgg + g[:, t] * g[:, t]
    with np.errstate(all="ignore"):
        mu0 = Sd / n
        U = Sgd - mu0 * Sg
        den = Sgg - Sg * Sg / n
        live = (U > 0.0) & (den > 0.0) & (mu0 > 0.0)
        beta[:] = mu0
        idx = np.nonzero(live)[0]
        if len(idx) == 0:
            return T, theta, beta, status
        d, g, valid, n, Sd, Sg, mu0 = d[idx], g[idx], valid[idx], n[idx], Sd[idx], Sg[idx], mu0[idx]
        th = U[idx] / den[idx]
        be = mu0 - th * Sg / n
        low = ~(be > 0.0)
        be = np.where(low, 1e-3 * mu0, be)
        th = np.where(low, (Sd - n * be) / Sg, th)
    cur = _lrt_eval(d, g, valid, th, be)
    st = np.where(cur["bad"], 1, 2).astype(np.int32)
    lam = np.full(len(idx), 1e-3)
    keys = ("cost", "mag", "g0", "g1", "a00", "a10", "a11", "bad")
    for _ in range(max_iter):
        act = np.nonzero(st == 2)[0]
        if len(act) == 0:
            break
        sub = {k: cur[k][act] for k in keys}
        d0, d1, ok = _lrt_solve(sub, lam[act])
        fail = act[~ok]
        lam[fail] *= 10.0
        st[fail[lam[fail] > 1e10]] = 1
        act, d0, d1 = act[ok], d0[ok], d1[ok]
        if len(act) == 0:
            continue
        sub = {k: cur[k][act] for k in keys}
        sc = np.maximum(np.abs(th[act]), np.abs(be[act]))
        u0, u1, ok0 = _lrt_solve(sub, 0.0)
        with np.errstate(invalid="ignore"):
            small = ok0 & (np.abs(u0) <= xtol * sc) & (np.abs(u1) <= xtol * sc)
        qt, qb = th[act] + d0, be[act] + d1
        nxt = _lrt_eval(d[act], g[act], valid[act], qt, qb)
        with np.errstate(invalid="ignore"):
            better = ~nxt["bad"] & (nxt["cost"] <= sub["cost"] + MLE_COST_SLACK * sub["mag"])
        up = act[better]
        th[up], be[up] = qt[better], qb[better]
        for k in keys:
            cur[k][up] = nxt[k][better]
        lam[up] = np.maximum(lam[up] * 0.1, 1e-12)
        down = act[~better]
        lam[down] *= 10.0
        st[down[lam[down] > 1e10]] = 1
        st[act[small]] = 0
    good = ~cur["bad"]
    s1, s2 = np.zeros(len(idx)), np.zeros(len(idx))
    with np.errstate(all="ignore"):
        for t in range(K * K):
            mu = th * g[:, t] + be
            pos = valid[:, t] & (d[:, t] > 0.0)
            s1 = s1 + np.where(pos, d[:, t] * np.log(np.where(pos, mu / mu0, 1.0)), 0.0)
            s2 = s2 + np.where(valid[:, t], mu, 0.0)
        t_ = 2.0 * s1 - 2.0 * (s2 - Sd)
    T[idx] = np.where(good & (t_ > 0.0), t_, 0.0)
    theta[idx] = np.where(good, th, 0.0)
    beta[idx] = np.where(good, be, mu0)
    status[idx] = st
    return T, theta, beta, status


def _check_lrt_args(shape, gain, offset, read_var, sigma0, radius, p_fa, min_distance, max_peaks_per_frame):
    """-> (profile e, the threshold rounded to float32 as a Python float)."""
    if len(shape) != 3:
        raise ValueError(f"movie must be [F, H, W], got {tuple(shape)}")
    if not (gain > 0 and math.isfinite(gain)):
        raise ValueError(f"gain must be finite and > 0, got {gain}")
    if not math.isfinite(offset):
        raise ValueError(f"offset must be finite, got {offset}")
    if not (read_var >= 0 and math.isfinite(read_var)):
        raise ValueError(f"read_var must be finite and >= 0, got {read_var}")
    e = psf_profile(sigma0, radius)
    r = len(e) // 2
    if shape[1] <= r or shape[2] <= r:
        raise ValueError(f"frames of {shape[1]} x {shape[2]} (H x W) are not larger than the radius {r}")
    if int(min_distance) != min_distance or not 1 <= min_distance <= 16:
        raise ValueError(f"min_distance must be an integer from 1 to 16, got {min_distance}")
    if int(max_peaks_per_frame) != max_peaks_per_frame or not 1 <= max_peaks_per_frame <= LRT_MAX_PEAKS:
        raise ValueError(f"max_peaks_per_frame must be an integer from 1 to {LRT_MAX_PEAKS}, got {max_peaks_per_frame}")
    return e, float(np.float32(detection_threshold(p_fa)))


def _check_detector(detector, localization=None):
    """detector= of the tracking functions -> the keyword arguments of the likelihood-ratio detector (camera keys missing
    from it are those of `localization`, the camera model of the fit, when that is given)."""
    if not isinstance(detector, dict) or set(detector) - set(_DETECTOR_DEFAULTS) - {"method"}:
        raise ValueError(f"detector must be None or a dict with keys among method, {', '.join(_DETECTOR_DEFAULTS)}, got "
                         f"{detector!r}")
    if detector.get("method") != "lrt":
        raise ValueError(f"detector['method'] must be 'lrt', got {detector.get('method')!r}")
    out = dict(_DETECTOR_DEFAULTS)
    out.update({k: v for k, v in (localization or {}).items() if k in ("gain", "offset", "read_var", "sigma0")})
    out.update({k: v for k, v in detector.items() if k != "method"})
    return out


def _lrt_detect_cuda(movie, e, thr, gain, offset, read_var, min_distance, max_peaks_per_frame, return_map):
    """Both stages on the GPU -> (count [F], coords [F, cap, 2], stats [F, cap, 4], status [F, cap], score map or None)."""
    from .. import ops
    movie = movie.float()
    if not bool(torch.isfinite(movie).all()):
        raise ValueError("movie must be finite")
    count, coords, values, smap = ops.score_peaks(movie, e, gain, offset, read_var, thr, int(min_distance),
                                                  int(max_peaks_per_frame), return_map)
    kept, kcoords, stats, status = ops.lrt_peaks(movie, e, gain, offset, read_var, thr, count, coords, values)
    return kept, kcoords, stats, status, smap


def _lrt_detect_numpy(arr, e, thr, gain, offset, read_var, min_distance, max_peaks_per_frame):
    """Both stages on the host for a float32 movie -> (list of F coords [n_f, 2] int64, list of F stats [n_f, 5] float64,
    score map [F, H, W] float32)."""
    if not np.isfinite(arr).all():
        raise ValueError("movie must be finite")
    smap = _score_numpy(arr, e, gain, offset, read_var)
    cand = []
    for f in range(len(smap)):
        c, n_cand = _peaks_numpy(smap[f], None, int(min_distance), absolute=np.float32(thr))
        if n_cand > max_peaks_per_frame:
            raise RuntimeError(f"a frame has {n_cand} peak candidates but max_peaks_per_frame = {max_peaks_per_frame}; raise "
                               f"max_peaks_per_frame (up to {LRT_MAX_PEAKS}) or lower p_fa")
        cand.append(c)
    fr = np.concatenate([np.full(len(c), f, np.int64) for f, c in enumerate(cand)]) if cand else np.zeros(0, np.int64)
    yx = np.concatenate(cand) if cand else np.zeros((0, 2), np.int64)
    T, theta, beta, status = _lrt_numpy(arr, e, gain, offset, read_var, fr, yx[:, 0], yx[:, 1])
    keep = T > thr
    table = np.stack([T, theta, beta - read_var, smap[fr, yx[:, 0], yx[:, 1]].astype(np.float64),
                      status.astype(np.float64)], axis=1)
    coords = [yx[(fr == f) & keep] for f in range(len(smap))]
    stats = [table[(fr == f) & keep] for f in range(len(smap))]
    return coords, stats, smap


def detect_particles_lrt_movie(movie, gain=1.0, offset=0.0, read_var=0.0, sigma0=1.0, radius=None, p_fa=1e-6, min_distance=3,
                               max_peaks_per_frame=512, return_map=True):
    """Likelihood-ratio detection of every frame of a movie [F, H, W] in camera units (photons = max((adu - offset) / gain,
    0), read_var the readout variance in photons^2, as fit_spots_mle): per pixel "local background only" against "background
    plus one spot of width sigma0 centred here" over the clipped (2 radius + 1)^2 window (radius from 1 to LRT_MAX_RADIUS,
    default ceil(3 sigma0)), at the per-pixel false-alarm probability p_fa in (0, 0.5].  Stage 1: the score statistic of
    every pixel and its local maxima above detection_threshold(p_fa) by the rule of detect_particles_movie (min_distance, at
    most max_peaks_per_frame candidates per frame or it raises).  Stage 2: the exact Poisson likelihood ratio T at those
    candidates; a detection has T above the same threshold -> (list of F coordinate arrays [n_f, 2] int64 (y, x) in stage-1
    order, list of F arrays [n_f, 5] float64 (T, photons, background per pixel, the stage-1 statistic, status: 0 converged, 1
    damping exhausted, 2 iteration cap, T then being a lower bound), the score map [F, H, W] float32 of the input's kind or
    None with return_map=False).  A CUDA tensor runs csrc/detect.hip, anything else the restatements _score_numpy and
    _lrt_numpy.  The threshold does not depend on the frame: an empty frame yields nothing, a bright spot hides no dim one."""
    gain, offset, read_var = float(gain), float(offset), float(read_var)
    e, thr = _check_lrt_args(movie.shape, gain, offset, read_var, sigma0, radius, p_fa, min_distance, max_peaks_per_frame)
    if _is_cuda(movie):
        kept, kcoords, stats, status, smap = _lrt_detect_cuda(movie, e, thr, gain, offset, read_var, min_distance,
                                                              max_peaks_per_frame, return_map)
        kept = kept.cpu().numpy()
        top = int(kept.max()) if len(kept) else 0
        kcoords = kcoords[:, :top].cpu().numpy().astype(np.int64)
        table = torch.cat([stats[:, :top], status[:, :top, None].double()], dim=2).cpu().numpy()
        return ([kcoords[f, :kept[f]] for f in range(len(kept))], [table[f, :kept[f]] for f in range(len(kept))], smap)
    was_tensor = torch.is_tensor(movie)
    arr = np.ascontiguousarray(movie.detach().numpy() if was_tensor else np.asarray(movie), dtype=np.float32)
    coords, stats, smap = _lrt_detect_numpy(arr, e, thr, gain, offset, read_var, min_distance, max_peaks_per_frame)
    if not return_map:
        return coords, stats, None
    return coords, stats, (torch.from_numpy(smap) if was_tensor else smap)


def detect_particles_lrt(image, gain=1.0, offset=0.0, read_var=0.0, sigma0=1.0, radius=None, p_fa=1e-6, min_distance=3):
    """detect_particles_lrt_movie of one frame [H, W] -> (coordinates [n, 2] (y, x), stats [n, 5], score map [H, W])."""
    if len(image.shape) != 2:
        raise ValueError(f"image must be [H, W], got {tuple(image.shape)}; use detect_particles_lrt_movie for a movie")
    coords, stats, smap = detect_particles_lrt_movie(image[None], gain, offset, read_var, sigma0, radius, p_fa, min_distance)
    return coords[0], stats[0], smap[0]


# ----------------------------------------------------------------------------------------------------------------------
# linking
# ----------------------------------------------------------------------------------------------------------------------
def link_particles(coords_t0, coords_t1, max_distance=15):
    """Reference link_particles: Hungarian assignment on the Euclidean distances, links longer than max_distance dropped ->
    (links [(i0, i1), ...], unlinked_t0, unlinked_t1)."""
    n0, n1 = len(coords_t0), len(coords_t1)
    if n0 == 0 or n1 == 0:
        return [], list(range(n0)), list(range(n1))
    from scipy.optimize import linear_sum_assignment
    c0, c1 = np.asarray(coords_t0), np.asarray(coords_t1)
    cost = np.sqrt(((c0[:, None, :] - c1[None, :, :]) ** 2).sum(axis=2)).astype(np.float64)
    rows, cols = linear_sum_assignment(cost, maximize=False)
    links = [(int(i), int(j)) for i, j in zip(rows, cols) if cost[i, j] <= max_distance]
    used0, used1 = {i for i, _ in links}, {j for _, j in links}
    return links, [i for i in range(n0) if i not in used0], [j for j in range(n1) if j not in used1]


def _link_tracks(all_coordinates, max_linking_distance, min_track_length, verbose=False):
    """The book-keeping of the reference's track_particles (:225-336) on per-frame coordinate arrays -> (tracks
    {id: [(frame, y, x), ...]} with sequential ids for tracks of >= min_track_length positions, detections as four int64
    arrays frame / y / x / track_id in the reference's row order, number of tracks before the length filter)."""
    tracks, active, rows = {}, {}, []          # active: track id -> (position, frame), in insertion order
    next_id = 0

    def start(frame, pos):
        nonlocal next_id
        tracks[next_id] = [(frame, pos[0], pos[1])]
        active[next_id] = (pos, frame)
        rows.append((frame, pos[0], pos[1], next_id))
        next_id += 1

    for frame, current in enumerate(all_coordinates):
        if frame == 0:
            for pos in current:
                start(0, pos)
            continue
        ids = list(active.keys())
        if ids and len(current) > 0:
            previous = np.array([active[i][0] for i in ids])
            links, _, fresh = link_particles(previous, current, max_distance=max_linking_distance)
            for i0, i1 in links:
                pos = current[i1]
                tracks[ids[i0]].append((frame, pos[0], pos[1]))
                active[ids[i0]] = (pos, frame)
                rows.append((frame, pos[0], pos[1], ids[i0]))
            for i1 in fresh:
                start(frame, current[i1])
            if verbose:
                print(f"Frame {frame}: {len(links)} links, {len(fresh)} new tracks")
        elif len(current) > 0:
            for pos in current:
                start(frame, pos)
        for i in [i for i, (_, last) in active.items() if last < frame]:       # a track that misses a frame ends
            del active[i]
    long_ids = sorted(i for i, t in tracks.items() if len(t) >= min_track_length)
    new_id = {old: new for new, old in enumerate(long_ids)}
    det = np.array(rows, dtype=np.int64).reshape(-1, 4)
    # the reference renumbers only the long tracks in the detections table; a short track keeps its first id
    det[:, 3] = [new_id.get(i, i) for i in det[:, 3]]
    return ({new_id[i]: tracks[i] for i in long_ids},
            {"frame": det[:, 0].copy(), "y": det[:, 1].copy(), "x": det[:, 2].copy(), "track_id": det[:, 3].copy()},
            len(tracks))


LINK_MAX_DETECTIONS = 1024   # per frame, the limit of csrc/linking.hip (ops.LINK_MAX_DETECTIONS)
LINK_MAX_GAP = 8             # missed frames a gap link may bridge (ops.LINK_MAX_GAP)


def _assign_pair_numpy(c0, c1):
    """The solver of csrc/linking.hip::lk_link_kernel on the host, same roles, same tie rule, same order of fp64 operations:
    exact rectangular assignment between c0 [n0, 2] and c1 [n1, 2] (integers, (y, x)) on the Euclidean distance by shortest
    augmenting paths with duals.  The side with fewer points plays rows (c0 on equality), rows are augmented in ascending
    index, and the closest unvisited column is the minimum of (path cost, column already matched, column index)
    -> (partner [n1] int64: index into c0 or -1, BEFORE the max_distance filter; distance [n1] float64 of each link)."""
    c0, c1 = np.asarray(c0, dtype=np.int64).reshape(-1, 2), np.asarray(c1, dtype=np.int64).reshape(-1, 2)
    n0, n1 = len(c0), len(c1)
    partner, dist = np.full(n1, -1, np.int64), np.zeros(n1)
    if n0 == 0 or n1 == 0:
        return partner, dist
    rows_prev = n0 <= n1
    R, C = (c0, c1) if rows_prev else (c1, c0)
    d = (R[:, None, :] - C[None, :, :]).astype(np.float64)
    cost = np.sqrt(d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1])
    nr, nc = cost.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    for cur in range(nr):
        spc, path = np.full(nc, np.inf), np.full(nc, -1, np.int64)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            SR[i] = True
            r = ((min_val + cost[i]) - u[i]) - v
            upd = ~SC & (r < spc)
            spc[upd] = r[upd]
            path[upd] = i
            low = spc[~SC].min()
            tie = np.flatnonzero(~SC & (spc == low))
            free = tie[row4col[tie] < 0]
            j = int(free[0]) if len(free) else int(tie[0])
            min_val = low
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
            SC[j] = True
        others = np.flatnonzero(SR)
        others = others[others != cur]
        u[others] = u[others] + (min_val - spc[col4row[others]])
        u[cur] = u[cur] + min_val
        v[SC] = v[SC] - (min_val - spc[SC])
        j = sink
        while True:
            r_ = int(path[j])
            row4col[j] = r_
            col4row[r_], j = j, int(col4row[r_])
            if r_ == cur:
                break
    if rows_prev:
        has = row4col >= 0
        partner[has] = row4col[has]
        dist[has] = cost[row4col[has], np.flatnonzero(has)]
    else:
        partner[:] = col4row
        dist[:] = cost[np.arange(nr), col4row]
    return partner, dist


def _padded_detections(coords, counts):
    """Per-frame coordinate arrays, or a padded [F, cap, 2] array with counts [F] -> (padded int32 [F, cap, 2], counts int32)."""
    if counts is None:
        frames = [np.asarray(c).reshape(-1, 2) for c in coords]
        counts = np.array([len(c) for c in frames], np.int32)
        cap = max(1, int(counts.max()) if len(frames) else 1)
        padded = np.zeros((len(frames), cap, 2), np.int32)
        for f, c in enumerate(frames):
            padded[f, :len(c)] = c
        return padded, counts
    if torch.is_tensor(coords):
        coords = coords.detach().cpu().numpy()
    if torch.is_tensor(counts):
        counts = counts.detach().cpu().numpy()
    padded, counts = np.asarray(coords), np.asarray(counts)
    if padded.ndim != 3 or padded.shape[2] != 2:
        raise ValueError(f"coords must be [F, cap, 2], got {tuple(padded.shape)}")
    if counts.shape != (padded.shape[0],):
        raise ValueError(f"counts must be [{padded.shape[0]}], got {tuple(counts.shape)}")
    if len(counts) and (counts.min() < 0 or counts.max() > padded.shape[1]):
        raise ValueError(f"counts must lie in 0 .. {padded.shape[1]}")
    return padded.astype(np.int32), counts.astype(np.int32)


def _check_movie_start(movie_start, F):
    if movie_start is None:
        return None
    ms = movie_start.detach().cpu().numpy() if torch.is_tensor(movie_start) else np.asarray(movie_start)
    if ms.shape != (F,):
        raise ValueError(f"movie_start must have one entry per frame, got {tuple(ms.shape)} for {F} frames")
    return ms != 0


def link_particles_movie(coords, counts=None, max_distance=15, movie_start=None):
    """link_particles for every pair of consecutive frames of a movie at once.  coords [F, cap, 2] (y, x) with counts [F], as
    ops.dog_peaks returns them, or (counts=None) a list of per-frame arrays [n_f, 2]; movie_start [F] (optional): a true entry
    opens a new movie, whose first frame gets no links -> link [F, cap] int32 of the input's kind: for every detection of
    frame f the index of its partner in frame f - 1, or -1.  CUDA tensors go to the kernel (ops.link_frames), anything else
    to its restatement (_assign_pair_numpy).  Every pair is solved in full in detection order and links longer than
    max_distance are dropped afterwards, as the reference does; where a pair has several optimal assignments the choice may
    differ from scipy's (link_particles), whose choice depends on the order of its rows."""
    if float(max_distance) != float(max_distance):
        raise ValueError("max_distance is NaN")
    if _is_cuda(coords):
        if counts is None or not _is_cuda(counts):
            raise ValueError("CUDA coords [F, cap, 2] need CUDA counts [F]")
        if coords.dim() != 3 or coords.shape[2] != 2:
            raise ValueError(f"coords must be [F, cap, 2], got {tuple(coords.shape)}")
        if coords.shape[1] > LINK_MAX_DETECTIONS:
            raise ValueError(f"{coords.shape[1]} detections per frame, the linking kernel's limit is {LINK_MAX_DETECTIONS} "
                             f"(LINK_MAX_DETECTIONS)")
        from .. import ops
        return ops.link_frames(coords.int(), counts.int(), float(max_distance), movie_start)
    as_tensor = torch.is_tensor(coords)
    padded, counts = _padded_detections(coords, counts)
    F, cap = padded.shape[:2]
    if cap > LINK_MAX_DETECTIONS:
        raise ValueError(f"{cap} detections per frame, the linking kernel's limit is {LINK_MAX_DETECTIONS} "
                         f"(LINK_MAX_DETECTIONS)")
    ms = _check_movie_start(movie_start, F)
    link = np.full((F, cap), -1, np.int32)
    for f in range(1, F):
        if ms is not None and ms[f]:
            continue
        partner, dist = _assign_pair_numpy(padded[f - 1, :counts[f - 1]], padded[f, :counts[f]])
        link[f, :counts[f]] = np.where((partner >= 0) & (dist <= max_distance), partner, -1)
    return torch.from_numpy(link) if as_tensor else link


def _check_max_gap(max_gap, allow_zero=False):
    lo = 0 if allow_zero else 1
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, float, np.integer, np.floating)) \
            or int(max_gap) != max_gap or not lo <= max_gap <= LINK_MAX_GAP:
        raise ValueError(f"max_gap must be an integer from {lo} to {LINK_MAX_GAP} (LINK_MAX_GAP), got {max_gap!r}")
    return int(max_gap)


def _close_gaps_numpy(padded, counts, link, max_gap, max_distance, ms):
    """csrc/linking.hip::gc_init_kernel / gc_pass_kernel on the host, pass by pass and frame by frame -> (gap_partner [F, cap]
    int32, gap_frames [F, cap] int32)."""
    F, cap = link.shape
    gap_partner, gap_frames = np.full((F, cap), -1, np.int32), np.zeros((F, cap), np.int32)
    has_succ, linked = np.zeros((F, cap), bool), np.zeros((F, cap), bool)
    for f in range(1, F):
        if ms is not None and ms[f]:
            continue
        l = link[f, :counts[f]].astype(np.int64)
        ok = (l >= 0) & (l < counts[f - 1])                   # a link outside the frame before counts as none
        linked[f, :counts[f]] = ok
        has_succ[f - 1, l[ok]] = True
    for g in range(2, max_gap + 2):                           # shortest gaps first
        for f in range(g, F):
            if ms is not None and ms[f - g + 1:f + 1].any():
                continue
            ends = np.flatnonzero(~has_succ[f - g, :counts[f - g]])
            starts = np.flatnonzero(~linked[f, :counts[f]] & (gap_frames[f, :counts[f]] == 0))
            partner, dist = _assign_pair_numpy(padded[f - g, ends], padded[f, starts])
            ok = (partner >= 0) & (dist <= max_distance)      # solve first, filter afterwards
            gap_partner[f, starts[ok]] = ends[partner[ok]]
            gap_frames[f, starts[ok]] = g
            has_succ[f - g, ends[partner[ok]]] = True
    return gap_partner, gap_frames


def close_gaps_movie(coords, counts, link, max_gap, max_distance=15, movie_start=None):
    """Gap closing after link_particles_movie: the end of a track is linked to the start of a later track across up to max_gap
    (1 .. LINK_MAX_GAP) missed frames.  coords [F, cap, 2] (y, x), counts [F], link [F, cap] -> (gap_partner [F, cap] int32,
    gap_frames [F, cap] int32) of the input's kind: detection (f, j) continues the track that ended at detection
    gap_partner[f, j] of frame f - gap_frames[f, j]; -1 and 0 everywhere else, beyond counts too.

    An open start is a detection with link < 0 and no gap link yet; an open end one that no detection of the next frame links
    to and no gap link points at yet.  Passes g = 2, 3, ..., max_gap + 1, shortest gaps first: for every frame f with
    f - g >= 0 and no movie_start flag in the frames f - g + 1 .. f, the full rectangular assignment between the open ends
    of frame f - g and the open starts of frame f (both in ascending detection index) is solved exactly as
    link_particles_movie solves a frame pair (_assign_pair_numpy), then pairs longer than max_distance are dropped: they stay
    open for the later passes, an accepted pair closes both its ends.  CUDA tensors go to the kernel (ops.close_gaps),
    anything else to its restatement."""
    max_gap = _check_max_gap(max_gap)
    if float(max_distance) != float(max_distance):
        raise ValueError("max_distance is NaN")
    if _is_cuda(coords):
        if not (_is_cuda(counts) and _is_cuda(link)):
            raise ValueError("CUDA coords [F, cap, 2] need CUDA counts [F] and a CUDA link [F, cap]")
        from .. import ops
        return ops.close_gaps(coords.int(), counts.int(), link.int(), max_gap, float(max_distance), movie_start)
    as_tensor = torch.is_tensor(coords)
    padded, counts = _padded_detections(coords, counts)
    F, cap = padded.shape[:2]
    if cap > LINK_MAX_DETECTIONS:
        raise ValueError(f"{cap} detections per frame, the linking kernel's limit is {LINK_MAX_DETECTIONS} "
                         f"(LINK_MAX_DETECTIONS)")
    link = link.detach().cpu().numpy() if torch.is_tensor(link) else np.asarray(link)
    if link.shape != (F, cap):
        raise ValueError(f"link must be [{F}, {cap}], got {tuple(link.shape)}")
    gp, gf = _close_gaps_numpy(padded, counts, link, max_gap, float(max_distance), _check_movie_start(movie_start, F))
    return (torch.from_numpy(gp), torch.from_numpy(gf)) if as_tensor else (gp, gf)


def _chain_numpy(link, counts, ms, gap_partner=None, gap_frames=None):
    """csrc/linking.hip::lk_chain_kernel (with gap tensors: lk_chain_gaps_kernel) on the host -> (ids [F, cap] int32, -1
    beyond counts; lengths [F * cap] int32, detections per track; number of tracks)."""
    F, cap = link.shape
    ids, lengths = np.full((F, cap), -1, np.int32), np.zeros(F * cap, np.int32)
    next_id, n_prev = 0, 0
    for f in range(F):
        n = int(counts[f])
        fresh = f == 0 or (ms is not None and ms[f])
        l = link[f, :n].astype(np.int64) if not fresh else np.full(n, -1, np.int64)
        l = np.where(l >= n_prev, -1, l)
        new = l < 0
        cur = np.where(new, 0, ids[f - 1, np.maximum(l, 0)] if f > 0 else 0)
        if gap_frames is not None and not fresh:
            g, p = gap_frames[f, :n].astype(np.int64), gap_partner[f, :n].astype(np.int64)
            ok = new & (g >= 2) & (g <= LINK_MAX_GAP + 1) & (f - g >= 0)
            src = np.where(ok, f - g, 0)
            ok &= (p >= 0) & (p < np.asarray(counts)[src])   # never read past the partner frame
            cur = np.where(ok, ids[src, np.where(ok, p, 0)], cur)
            new = new & ~ok
        cur = np.where(new, next_id + np.cumsum(new) - 1, cur)
        ids[f, :n] = cur
        lengths[cur] = np.where(new, 1, lengths[cur] + 1)
        next_id += int(new.sum())
        n_prev = n
    return ids, lengths, next_id


def chain_tracks(link, counts, movie_start=None, gap_partner=None, gap_frames=None):
    """Track ids from the links of link_particles_movie: a linked detection inherits its partner's id, an unlinked one takes
    the next free id in ascending detection index, frame 0 (and every movie_start frame) starts one track per detection: the
    numbering of the reference's track_particles.  link [F, cap], counts [F] -> (ids [F, cap] int32, -1 beyond counts;
    lengths [F * cap] int32, the number of positions of track i at index i; n_tracks [1] int32) of the input's kind.  CUDA
    tensors go to the kernel (ops.chain_tracks).  With gap_partner / gap_frames [F, cap] (close_gaps_movie) an unlinked
    detection with gap_frames = g > 0 inherits the id of detection gap_partner of frame f - g instead of opening a track;
    lengths counts detections, not the rows fill_gaps adds."""
    if (gap_partner is None) != (gap_frames is None):
        raise ValueError("gap_partner and gap_frames must both be given or both be None")
    if _is_cuda(link):
        if not _is_cuda(counts):
            raise ValueError("a CUDA link tensor needs CUDA counts")
        from .. import ops
        if gap_partner is None:
            return ops.chain_tracks(link.int(), counts.int(), movie_start)
        if not (_is_cuda(gap_partner) and _is_cuda(gap_frames)):
            raise ValueError("a CUDA link tensor needs CUDA gap_partner and gap_frames")
        return ops.chain_tracks(link.int(), counts.int(), movie_start, gap_partner.int(), gap_frames.int())
    as_tensor = torch.is_tensor(link)
    link = link.detach().numpy() if as_tensor else np.asarray(link)
    counts = counts.detach().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if link.ndim != 2:
        raise ValueError(f"link must be [F, cap], got {tuple(link.shape)}")
    F, cap = link.shape
    if counts.shape != (F,):
        raise ValueError(f"counts must be [{F}], got {tuple(counts.shape)}")
    if F and (counts.min() < 0 or counts.max() > cap):
        raise ValueError(f"counts must lie in 0 .. {cap}")
    if gap_partner is not None:
        gap_partner = gap_partner.detach().cpu().numpy() if torch.is_tensor(gap_partner) else np.asarray(gap_partner)
        gap_frames = gap_frames.detach().cpu().numpy() if torch.is_tensor(gap_frames) else np.asarray(gap_frames)
        if gap_partner.shape != (F, cap) or gap_frames.shape != (F, cap):
            raise ValueError(f"gap_partner and gap_frames must be [{F}, {cap}]")
    ids, lengths, n = _chain_numpy(link, counts, _check_movie_start(movie_start, F), gap_partner, gap_frames)
    n = np.array([n], np.int32)
    return (torch.from_numpy(ids), torch.from_numpy(lengths), torch.from_numpy(n)) if as_tensor else (ids, lengths, n)


def _detections_table(coords, counts, ids, lengths, min_track_length):
    """The detections table from chained ids, torch ops on the tensors' device: coords [F, cap, 2], counts [F], ids [F, cap],
    lengths [>= tracks] -> (frame, y, x, track_id, in_long_track), int64 / bool [N], in the reference's row order: frames
    ascending and, within a frame, ascending id as handed out (linked detections in the order of their tracks, then the new
    ones in detection order: new ids are larger than every older one).  Tracks of at least min_track_length positions are
    renumbered 0, 1, ... in ascending first id; a shorter track keeps its first id in the table, as in the reference."""
    F, cap = ids.shape
    valid = torch.arange(cap, device=ids.device)[None, :] < counts[:, None]
    fr, j = valid.nonzero(as_tuple=True)
    tid = ids[fr, j].long()
    order = torch.argsort(fr * (lengths.numel() + 1) + tid, stable=True)
    fr, j, tid = fr[order], j[order], tid[order]
    is_long = (lengths > 0) & (lengths >= min_track_length)
    new_id = torch.cumsum(is_long, 0) - 1
    in_long = is_long[tid]
    return fr, coords[fr, j, 0].long(), coords[fr, j, 1].long(), torch.where(in_long, new_id[tid], tid), in_long


def fill_gaps(coords, counts, ids, lengths, gap_partner, gap_frames, min_track_length=1):
    """_detections_table with the frames a gap link bridges filled in, torch ops on the tensors' device: coords [F, cap, 2],
    counts [F], ids [F, cap] and lengths from chain_tracks(..., gap_partner, gap_frames) -> (frame, y, x, track_id,
    in_long_track, filled), int64 / bool [N].  A gap link from detection gap_partner[f, j] of frame f - g at (y0, x0) to
    detection (f, j) at (y1, x1) adds the rows of the frames f - g + k, k = 1 .. g - 1, at rint(y0 + (y1 - y0) * k / g) and the
    same for x (float64, round-half-to-even, the rounding of extract_patches_flat), with the track's id and filled = True.
    Rows are in the table's order, frames ascending and ascending id within a frame, so every track is contiguous in frames:
    msd.track_msd and track_sequences take the filled table as it is.  Tracks of at least min_track_length DETECTIONS (lengths
    does not count the added rows) are renumbered as _detections_table renumbers them."""
    F, cap = ids.shape
    dev = ids.device
    valid = torch.arange(cap, device=dev)[None, :] < counts[:, None]
    fr, j = valid.nonzero(as_tuple=True)
    tid = ids[fr, j].long()
    y, x = coords[fr, j, 0].long(), coords[fr, j, 1].long()
    g = gap_frames[fr, j].long()
    has = g > 1
    sf, sg, stid = fr[has], g[has], tid[has]
    f0 = (sf - sg).clamp_min(0)
    p = gap_partner[sf, j[has]].long().clamp(0, cap - 1)
    y0, x0 = coords[f0, p, 0].double(), coords[f0, p, 1].double()
    y1, x1 = y[has].double(), x[has].double()
    n_add = sg - 1
    which = torch.repeat_interleave(torch.arange(len(sg), device=dev), n_add)
    k = torch.arange(len(which), device=dev) - (torch.cumsum(n_add, 0) - n_add)[which] + 1
    kd, gd = k.double(), sg[which].double()
    fy = torch.round(y0[which] + (y1[which] - y0[which]) * kd / gd).long()
    fx = torch.round(x0[which] + (x1[which] - x0[which]) * kd / gd).long()
    fr = torch.cat([fr, f0[which] + k])
    y, x, tid = torch.cat([y, fy]), torch.cat([x, fx]), torch.cat([tid, stid[which]])
    filled = torch.cat([torch.zeros(len(j), dtype=torch.bool, device=dev), torch.ones(len(which), dtype=torch.bool, device=dev)])
    order = torch.argsort(fr * (lengths.numel() + 1) + tid, stable=True)
    fr, y, x, tid, filled = fr[order], y[order], x[order], tid[order], filled[order]
    is_long = (lengths > 0) & (lengths >= min_track_length)
    new_id = torch.cumsum(is_long, 0) - 1
    in_long = is_long[tid]
    return fr, y, x, torch.where(in_long, new_id[tid], tid), in_long, filled


def _check_gap_args(max_gap, max_gap_distance, max_linking_distance):
    max_gap = _check_max_gap(max_gap, allow_zero=True)
    dist = max_linking_distance if max_gap_distance is None else max_gap_distance
    if float(dist) != float(dist):
        raise ValueError("max_gap_distance is NaN")
    return max_gap, float(dist)


def track_particles_tensors(movie, sigma1=1.0, sigma2=2.0, threshold_percentage=0.1, min_distance=3,
                            max_linking_distance=15, min_track_length=3, max_peaks_per_frame=512, movie_start=None,
                            return_dog=True, max_gap=0, max_gap_distance=None, detector=None):
    """Detection, linking, chaining, length filter and renumbering of a CUDA movie [F, H, W] without a copy of the
    coordinates to the host -> (dict of CUDA tensors frame, y, x, track_id (int64 [N], the reference's detections table in its
    row order), in_long_track (bool [N]: the rows whose track has >= min_track_length positions and so carries a renumbered
    id), n_tracks ([1] int32, before the length filter); DoG movie or None).  frame / y / x of the rows with in_long_track feed
    extract_patches_flat and refine_localizations as they are.  movie_start [F] marks the first frames of several movies
    concatenated along F.  max_gap > 0 (up to LINK_MAX_GAP) closes gaps of up to that many missed frames within
    max_gap_distance pixels (default: max_linking_distance; close_gaps_movie) and fills them (fill_gaps): the dict gains
    filled (bool [N], the interpolated rows), and min_track_length keeps counting detections.  detector (default None: the
    difference of Gaussians, the code path without it): {"method": "lrt"} with any of gain, offset, read_var, sigma0, radius
    and p_fa, the arguments of detect_particles_lrt_movie, which then detects (csrc/detect.hip, both stages on the device);
    sigma1, sigma2 and threshold_percentage are unused and the second result is the score map."""
    if not _is_cuda(movie):
        raise ValueError("track_particles_tensors needs a CUDA movie; use track_particles_flat(..., linking='device') on the host")
    max_gap, gap_distance = _check_gap_args(max_gap, max_gap_distance, max_linking_distance)
    if detector is not None:
        det = _check_detector(detector)
        gain, offset, read_var = float(det["gain"]), float(det["offset"]), float(det["read_var"])
        e, thr = _check_lrt_args(movie.shape, gain, offset, read_var, det["sigma0"], det["radius"], det["p_fa"], min_distance,
                                 max_peaks_per_frame)
    else:
        w1, w2 = _check_detection_args(movie.shape, sigma1, sigma2, min_distance)
    if max_peaks_per_frame > LINK_MAX_DETECTIONS:
        raise ValueError(f"max_peaks_per_frame = {max_peaks_per_frame}, the linking kernel's limit is {LINK_MAX_DETECTIONS} "
                         f"(LINK_MAX_DETECTIONS)")
    from .. import ops
    if detector is not None:
        count, coords, _, _, dog = _lrt_detect_cuda(movie, e, thr, gain, offset, read_var, min_distance, max_peaks_per_frame,
                                                    return_dog)
    else:
        count, coords, _, dog = ops.dog_peaks(movie.float(), w1, w2, threshold_percentage, int(min_distance),
                                              max_peaks_per_frame, return_dog)
    link = ops.link_frames(coords, count, float(max_linking_distance), movie_start)
    if max_gap > 0:
        gap_partner, gap_frames = ops.close_gaps(coords, count, link, max_gap, gap_distance, movie_start)
        ids, lengths, n_tracks = ops.chain_tracks(link, count, movie_start, gap_partner, gap_frames)
        fr, y, x, tid, in_long, filled = fill_gaps(coords, count, ids, lengths, gap_partner, gap_frames, min_track_length)
        return {"frame": fr, "y": y, "x": x, "track_id": tid, "in_long_track": in_long, "filled": filled,
                "n_tracks": n_tracks}, dog
    ids, lengths, n_tracks = ops.chain_tracks(link, count, movie_start)
    fr, y, x, tid, in_long = _detections_table(coords, count, ids, lengths, min_track_length)
    return {"frame": fr, "y": y, "x": x, "track_id": tid, "in_long_track": in_long, "n_tracks": n_tracks}, dog


def _tracks_from_table(fr, y, x, tid, in_long):
    """The tracks dictionary {id: [(frame, y, x), ...]} of the long tracks from the detections table (host arrays)."""
    fr, y, x, tid = fr[in_long], y[in_long], x[in_long], tid[in_long]
    order = np.argsort(tid, kind="stable")                           # rows are in frame order already
    fr, y, x, tid = fr[order], y[order], x[order], tid[order]
    cuts = np.flatnonzero(np.diff(tid)) + 1
    starts, ends = np.concatenate([[0], cuts]), np.concatenate([cuts, [len(tid)]])
    frames = fr.tolist()
    return {int(tid[a]): list(zip(frames[a:b], y[a:b], x[a:b])) for a, b in zip(starts, ends) if b > a}


def _detect_movie(movie, sigma1, sigma2, threshold_percentage, min_distance, max_peaks_per_frame, detector):
    """(coordinates per frame, DoG movie) of detect_particles_movie, or with a detector those of detect_particles_lrt_movie
    and its score map."""
    if detector is None:
        return detect_particles_movie(movie, sigma1, sigma2, threshold_percentage, min_distance, max_peaks_per_frame)
    det = _check_detector(detector)
    coords, _, smap = detect_particles_lrt_movie(movie, min_distance=min_distance, max_peaks_per_frame=max_peaks_per_frame,
                                                 **det)
    return coords, smap


def _track_device(movie, sigma1, sigma2, threshold_percentage, min_distance, max_linking_distance, min_track_length, verbose,
                  max_peaks_per_frame, max_gap=0, gap_distance=None, detector=None):
    """track_particles_flat with linking="device": the kernels for a CUDA movie, their restatements for anything else."""
    filled = None
    if _is_cuda(movie):
        t, dog = track_particles_tensors(movie, sigma1, sigma2, threshold_percentage, min_distance, max_linking_distance,
                                         min_track_length, max_peaks_per_frame, max_gap=max_gap, max_gap_distance=gap_distance,
                                         detector=detector)
        keys = ("frame", "y", "x", "track_id", "in_long_track") + (("filled",) if max_gap > 0 else ())
        packed = torch.stack([t[k].long() for k in keys]).cpu().numpy()          # the one copy to the host
        fr, y, x, tid, in_long = packed[0], packed[1], packed[2], packed[3], packed[4].astype(bool)
        if max_gap > 0:
            filled = packed[5].astype(bool)
        n_all = int(t["n_tracks"])
    else:
        coords, dog = _detect_movie(movie, sigma1, sigma2, threshold_percentage, min_distance, max_peaks_per_frame, detector)
        padded, counts = _padded_detections(coords, None)
        link = link_particles_movie(padded, counts, max_linking_distance)
        if max_gap > 0:
            gp, gf = _close_gaps_numpy(padded, counts, link, max_gap, gap_distance, None)
            ids, lengths, n_all = _chain_numpy(link, counts, None, gp, gf)
            fr, y, x, tid, in_long, filled = (a.numpy() for a in fill_gaps(
                torch.from_numpy(padded), torch.from_numpy(counts), torch.from_numpy(ids), torch.from_numpy(lengths),
                torch.from_numpy(gp), torch.from_numpy(gf), min_track_length))
        else:
            ids, lengths, n_all = _chain_numpy(link, counts, None)
            fr, y, x, tid, in_long = (a.numpy() for a in _detections_table(
                torch.from_numpy(padded), torch.from_numpy(counts), torch.from_numpy(ids), torch.from_numpy(lengths),
                min_track_length))
    if verbose:
        per_frame = np.bincount(fr, minlength=len(movie))
        for f, n in enumerate(per_frame):
            print(f"Frame {f}: {n} particles detected")
    det = {"frame": fr.copy(), "y": y.copy(), "x": x.copy(), "track_id": tid.copy()}
    if filled is not None:
        det["filled"] = filled.copy()
    return _tracks_from_table(fr, y, x, tid, in_long), det, dog, n_all


def track_particles_flat(image_sequence, sigma1=1.0, sigma2=2.0, threshold_percentage=0.1, min_distance=3,
                         max_linking_distance=15, min_track_length=3, verbose=False, max_peaks_per_frame=512, linking="host",
                         max_gap=0, max_gap_distance=None, detector=None):
    """track_particles without pandas: (tracks, detections as a dict of int64 arrays frame / y / x / track_id, DoG movie
    [F, H, W]).  linking="host" (default): scipy's assignment per frame in a loop on the host, rows in the order of the
    reference's active tracks.  linking="device": all frame pairs in one launch of csrc/linking.hip and the ids chained on the
    device for a CUDA movie (one copy to the host, for the dictionaries), the kernels' restatement for a host movie; same
    result wherever every frame pair has a single optimal assignment (see link_particles_movie).  max_gap > 0 (with
    linking="device" only) closes gaps of up to max_gap missed frames within max_gap_distance pixels (default:
    max_linking_distance) and fills them with interpolated positions: tracks and detections include the filled rows, and the
    detections gain the bool column filled.  detector (default None: the difference of Gaussians): {"method": "lrt", ...} as
    track_particles_tensors, with either linking; the third result is then the score map."""
    if linking not in ("host", "device"):
        raise ValueError(f"linking must be 'host' or 'device', got {linking!r}")
    max_gap, gap_distance = _check_gap_args(max_gap, max_gap_distance, max_linking_distance)
    if max_gap > 0 and linking != "device":
        raise ValueError(f"max_gap = {max_gap} needs linking=\"device\": the host loop links frame to frame only")
    movie = image_sequence
    if not torch.is_tensor(movie) and not isinstance(movie, np.ndarray):
        movie = np.stack([np.asarray(f) for f in movie])
    if linking == "device":
        tracks, det, dog, n_all = _track_device(movie, sigma1, sigma2, threshold_percentage, min_distance,
                                                max_linking_distance, min_track_length, verbose, max_peaks_per_frame,
                                                max_gap, gap_distance, detector)
        print(f"Tracking complete: {n_all} total tracks, {len(tracks)} tracks with ≥{min_track_length} frames")
        return tracks, det, dog
    coords, dog = _detect_movie(movie, sigma1, sigma2, threshold_percentage, min_distance, max_peaks_per_frame, detector)
    if verbose:
        for f, c in enumerate(coords):
            print(f"Frame {f}: {len(c)} particles detected")
    tracks, det, n_all = _link_tracks(coords, max_linking_distance, min_track_length, verbose)
    print(f"Tracking complete: {n_all} total tracks, {len(tracks)} tracks with ≥{min_track_length} frames")
    return tracks, det, dog


def track_particles(image_sequence, sigma1=1.0, sigma2=2.0, threshold_percentage=0.1, min_distance=3,
                    max_linking_distance=15, min_track_length=3, verbose=False, linking="host", max_gap=0,
                    max_gap_distance=None):
    """Reference track_particles -> (tracks {id: [(frame, y, x), ...]}, all_detections DataFrame with columns frame, y, x,
    track_id, filtered_images: the DoG movie [F, H, W], one image per frame when iterated).  Detection runs for the whole
    movie at once; linking, max_gap and max_gap_distance as in track_particles_flat (with max_gap > 0 the DataFrame gains the
    column filled)."""
    import pandas as pd
    tracks, det, dog = track_particles_flat(image_sequence, sigma1, sigma2, threshold_percentage, min_distance,
                                            max_linking_distance, min_track_length, verbose, linking=linking,
                                            max_gap=max_gap, max_gap_distance=max_gap_distance)
    return tracks, pd.DataFrame(det, columns=["frame", "y", "x", "track_id"] + (["filled"] if "filled" in det else [])), dog


def analyze_microscopy_sequence(image_sequence, sigma1=1.0, sigma2=2.0, threshold_percentage=0.1, min_distance=3,
                                max_linking_distance=15, min_track_length=3, visualize=False, verbose=False,
                                output_prefix=None, linking="host", max_gap=0, max_gap_distance=None):
    """Reference analyze_microscopy_sequence: track_particles, and with output_prefix the files <prefix>_detections.csv and
    <prefix>_tracks.pkl.  Plotting is not part of this package: visualize defaults to False and True raises."""
    if visualize:
        raise NotImplementedError("visualize=True needs the reference's visualize_tracks (helpers/helpersTracking.py), "
                                  "which this package does not restate; plot the returned tracks yourself")
    tracks, all_detections, filtered = track_particles(image_sequence, sigma1=sigma1, sigma2=sigma2,
                                                       threshold_percentage=threshold_percentage, min_distance=min_distance,
                                                       max_linking_distance=max_linking_distance,
                                                       min_track_length=min_track_length, verbose=verbose,
                                                       linking=linking, max_gap=max_gap,
                                                       max_gap_distance=max_gap_distance)
    if output_prefix:
        import pickle
        all_detections.to_csv(f"{output_prefix}_detections.csv", index=False)
        with open(f"{output_prefix}_tracks.pkl", "wb") as fh:
            pickle.dump(tracks, fh)
        print(f"Results saved with prefix: {output_prefix}")
    return tracks, all_detections, filtered


# ----------------------------------------------------------------------------------------------------------------------
# sub-pixel localisation
# ----------------------------------------------------------------------------------------------------------------------
def extract_patches_flat(movie, frames, ys, xs, patch_size=7):
    """One gather for all localisations of all tracks: movie [F, H, W] array / tensor, frames / ys / xs [N] -> patches
    [N, patch_size, patch_size] of the movie's kind and dtype, centred on the rounded positions (round-half-to-even), pixels
    outside the frame read as 0: extract_particle_patches without the dictionaries."""
    if patch_size % 2 != 1:
        raise ValueError("patch_size must be an odd number")
    is_np = not torch.is_tensor(movie)
    img = torch.as_tensor(np.asarray(movie)) if is_np else movie
    if img.dim() != 3:
        raise ValueError(f"movie must be [F, H, W], got {tuple(img.shape)}")
    _, H, W = img.shape
    half = patch_size // 2
    if _is_cuda(frames) and _is_cuda(ys) and _is_cuda(xs):       # positions already on the device (track_particles_tensors)
        fr = frames.to(img.device, torch.int64)
        yy, xx = torch.round(ys.double()).to(img.device, torch.int64), torch.round(xs.double()).to(img.device, torch.int64)
    else:
        fr = torch.as_tensor(np.asarray(frames).astype(np.int64), device=img.device)
        yy = torch.as_tensor(np.rint(np.asarray(ys, dtype=np.float64)).astype(np.int64), device=img.device)
        xx = torch.as_tensor(np.rint(np.asarray(xs, dtype=np.float64)).astype(np.int64), device=img.device)
    if not (len(fr) == len(yy) == len(xx)):
        raise ValueError("frames, ys and xs must have one entry per localisation")
    off = torch.arange(-half, half + 1, device=img.device)
    py, px = yy[:, None] + off[None, :], xx[:, None] + off[None, :]
    ok = ((py >= 0) & (py < H))[:, :, None] & ((px >= 0) & (px < W))[:, None, :]
    g = img[fr[:, None, None], py.clamp(0, H - 1)[:, :, None], px.clamp(0, W - 1)[:, None, :]]
    g = torch.where(ok, g, torch.zeros((), dtype=img.dtype, device=img.device))
    return g.numpy() if is_np else g


def _fit_normal(patch, p):
    """Residual sum of squares, J^T r and J^T J of the model at p [n, 5] for patches [n, P, P] float64."""
    n, P, _ = patch.shape
    ix, iy = np.arange(P, dtype=np.float64)[None, None, :], np.arange(P, dtype=np.float64)[None, :, None]
    c = [p[:, k, None, None] for k in range(5)]
    with np.errstate(all="ignore"):
        dx, dy = ix - c[1], iy - c[2]
        r2 = dx * dx + dy * dy
        s2 = c[3] * c[3]
        s3 = s2 * c[3]
        e = np.exp(-(r2 / (2.0 * s2)))
        ae = c[0] * e
        r = ((c[4] + ae) - patch).reshape(n, -1)
        J = np.stack([e, ae * dx / s2, ae * dy / s2, ae * r2 / s3, np.ones_like(e)], axis=1).reshape(n, 5, -1)
        return (r * r).sum(axis=1), np.einsum("nip,np->ni", J, r), np.einsum("nip,njp->nij", J, J)


def _fit_solve(A, g, lam):
    """(A + lam diag(A)) d = -g by Cholesky for every patch -> (d [n, 5], ok [n])."""
    n = len(g)
    L = np.zeros((n, 5, 5))
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for i in range(5):
            for j in range(i + 1):
                s = A[:, i, j].copy()
                if i == j:
                    s = s + lam * s
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                if i == j:
                    ok &= (s > 0.0) & (s < 1e300)
                    L[:, i, i] = np.sqrt(np.where(ok, s, 1.0))
                else:
                    L[:, i, j] = s / L[:, j, j]
        z = np.zeros((n, 5))
        for i in range(5):
            s = -g[:, i]
            for k in range(i):
                s = s - L[:, i, k] * z[:, k]
            z[:, i] = s / L[:, i, i]
        d = np.zeros((n, 5))
        for i in range(4, -1, -1):
            s = z[:, i]
            for k in range(i + 1, 5):
                s = s - L[:, k, i] * d[:, k]
            d[:, i] = s / L[:, i, i]
    return d, ok


def _refine_numpy(patches, xtol=FIT_XTOL, max_iter=FIT_MAX_ITER):
    """The fit of csrc/tracking.hip::rg_kernel for patches [N, P, P] on the host, all patches side by side -> (params [N, 5]
    float64 (amplitude, x0, y0, sigma, offset), peak [N] = patch.max() in the patches' dtype, status [N] int32)."""
    raw = np.asarray(patches)
    N, P, _ = raw.shape
    x = raw.astype(np.float64)
    flat = raw.reshape(N, -1)
    peak = flat.max(axis=1) if N else flat[:, 0]
    p = np.stack([x.reshape(N, -1).max(axis=1), np.full(N, float(P // 2)), np.full(N, float(P // 2)), np.ones(N),
                  x.reshape(N, -1).min(axis=1)], axis=1) if N else np.zeros((0, 5))
    status = np.full(N, 2, np.int32)
    if N == 0:
        return p, peak, status
    cost, g, A = _fit_normal(x, p)
    status[~(cost < 1e300)] = 3
    lam = np.full(N, 1e-3)
    for _ in range(max_iter):
        act = np.nonzero(status == 2)[0]
        if len(act) == 0:
            break
        d, ok = _fit_solve(A[act], g[act], lam[act])
        bad = act[~ok]
        lam[bad] *= 10.0
        status[bad[lam[bad] > 1e10]] = 1
        act, d = act[ok], d[ok]
        if len(act) == 0:
            continue
        pa = p[act]
        a0, a4 = np.abs(pa[:, 0]), np.abs(pa[:, 4])
        scale = np.stack([a0, np.maximum(np.abs(pa[:, 1]), 1.0), np.maximum(np.abs(pa[:, 2]), 1.0), np.abs(pa[:, 3]),
                          np.maximum(a4, a0)], axis=1)
        d0, ok0 = _fit_solve(A[act], g[act], 0.0)                 # the undamped step measures the distance to the optimum
        with np.errstate(invalid="ignore"):
            small = ok0 & (np.abs(d0) <= xtol * scale).all(axis=1)
        q = pa + d
        cq, gq, Aq = _fit_normal(x[act], q)
        # accepted unless the cost rises by more than its own rounding error: close to the optimum a step changes the cost by
        # less than that, and a strict test would stop the iteration at sqrt(eps) of the parameters
        with np.errstate(invalid="ignore"):
            better = cq <= cost[act] * FIT_COST_SLACK
        up = act[better]
        p[up], cost[up], g[up], A[up] = q[better], cq[better], gq[better], Aq[better]
        lam[up] = np.maximum(lam[up] * 0.1, 1e-12)
        down = act[~better]
        lam[down] *= 10.0
        status[down[lam[down] > 1e10]] = 1
        status[act[small]] = 0
    return p, peak, status


def refine_gaussian_patches(patches, xtol=FIT_XTOL):
    """Five-parameter Gaussian fit of patches [N, P, P] (P odd, 3 .. 15): CUDA float tensors go to the kernel
    (ops.refine_gaussian), anything else to the host restatement -> (params [N, 5] float64, peak [N], status [N] int32) of
    the input's kind."""
    if len(patches.shape) != 3 or patches.shape[1] != patches.shape[2]:
        raise ValueError(f"patches must be [N, P, P], got {tuple(patches.shape)}")
    P = patches.shape[1]
    if P % 2 != 1 or not 3 <= P <= 15:
        raise ValueError(f"patch side must be odd and from 3 to 15, got {P}")
    if not 0 < xtol <= 1.49012e-8:
        raise ValueError(f"xtol must be in (0, 1.49012e-8], got {xtol}")
    if _is_cuda(patches):
        from .. import ops
        return ops.refine_gaussian(patches.float(), xtol)
    if torch.is_tensor(patches):
        p, peak, st = _refine_numpy(patches.detach().numpy(), xtol)
        return torch.from_numpy(p), torch.from_numpy(np.ascontiguousarray(peak)), torch.from_numpy(st)
    return _refine_numpy(patches, xtol)


# ----------------------------------------------------------------------------------------------------------------------
# Poisson maximum-likelihood fit with Cramer-Rao bounds (csrc/localize.hip)
# ----------------------------------------------------------------------------------------------------------------------
MLE_MIN_SIGMA = 0.2       # the fitted width stays in (MLE_MIN_SIGMA, P)
MLE_COST_SLACK = 1e-13    # FIT_COST_SLACK - 1, of 2 sum(mu + d) instead of the cost
_SQRT2, _SQRT_2PI = 1.4142135623730951, 2.5066282746310002
_erf = np.frompyfunc(math.erf, 1, 1)


def _mle_data(raw, gain, offset, read_var):
    """Camera units -> photons: max((patch - offset) / gain, 0) + read_var, float64."""
    with np.errstate(invalid="ignore"):
        e = (raw.astype(np.float64) - offset) / gain
        return np.where(e > 0.0, e, 0.0) + read_var


def _mle_axis(P, c, s, fs):
    """The three tables of one axis for centres c [n] and widths s [n] -> E, dE/dc, dE/ds, each [P, n] (ml_axis)."""
    w, nc = _SQRT2 * s, 1.0 / (_SQRT_2PI * s)
    ns = nc / s
    t = [(float(k) - 0.5) - c for k in range(P + 1)]
    u = [tk / w for tk in t]
    e = [_erf(uk).astype(np.float64) for uk in u]
    g = [np.exp(-(uk * uk)) for uk in u]
    E = np.stack([0.5 * (e[k + 1] - e[k]) for k in range(P)])
    dc = np.stack([(g[k] - g[k + 1]) * nc for k in range(P)])
    ds = np.stack([(t[k] * g[k] - t[k + 1] * g[k + 1]) * ns for k in range(P)]) if fs else np.zeros_like(E)
    return E, dc, ds


def _mle_normal(d, p, read_var, fs):
    """Deviance, gradient, Fisher matrix, the out-of-domain flag and 2 sum(mu + d), the magnitude the deviance's rounding
    error scales with, of the model at p [n, 5] for data d [n, P, P] in photons (ml_eval of csrc/localize.hip: the same sums
    in the same order, pixel by pixel)."""
    n, P, _ = d.shape
    cost, mag, g, A = np.zeros(n), np.zeros(n), np.zeros((n, 5)), np.zeros((n, 5, 5))
    with np.errstate(all="ignore"):
        bad = ~(p[:, 0] > 0.0) | ~(p[:, 3] > MLE_MIN_SIGMA) | ~(p[:, 3] < float(P))
        ok = ~bad
        q = np.where(ok[:, None], p, np.array([1.0, 0.0, 0.0, 1.0, 1.0]))        # placeholders: their rows are zeroed below
        Ex, dEx, sEx = _mle_axis(P, q[:, 1], q[:, 3], fs)
        Ey, dEy, sEy = _mle_axis(P, q[:, 2], q[:, 3], fs)
        nonpos = np.zeros(n, bool)
        one = np.ones(n)
        for iy in range(P):
            nEy, ndEy, nsEy = q[:, 0] * Ey[iy], q[:, 0] * dEy[iy], q[:, 0] * sEy[iy]
            for ix in range(P):
                mu = (q[:, 4] + nEy * Ex[ix]) + read_var
                nonpos |= ~(mu > 0.0)
                dd = d[:, iy, ix]
                rm = 1.0 / mu
                r = dd * rm
                cost = cost + np.where(dd > 0.0, (mu - dd) + dd * np.log(np.where(dd > 0.0, r, 1.0)), mu)
                mag = mag + (mu + dd)
                J = (Ex[ix] * Ey[iy], nEy * dEx[ix], ndEy * Ex[ix], nEy * sEx[ix] + nsEy * Ex[ix], one)
                w = 1.0 - r
                for i in range(5):
                    g[:, i] = g[:, i] + J[i] * w
                    Jr = J[i] * rm
                    for j in range(i + 1):
                        A[:, i, j] = A[:, i, j] + Jr * J[j]
        cost, mag = 2.0 * cost, 2.0 * mag
        if not fs:
            A[:, 3, 3] = 1.0
        cost[bad], mag[bad], g[bad], A[bad] = 0.0, 0.0, 0.0, 0.0
    return cost, g, A, bad | (ok & nonpos), mag


def _mle_crlb(A):
    """Diagonal of A^-1 through the Cholesky factor (csrc/spot_fit.h::sf_crlb<5>) -> (variances [n, 5], ok [n])."""
    n = len(A)
    L = np.zeros((n, 5, 5))
    ok = np.ones(n, bool)
    v = np.zeros((n, 5))
    with np.errstate(all="ignore"):
        for i in range(5):
            for j in range(i + 1):
                s = A[:, i, j].copy()
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                if i == j:
                    ok &= (s > 0.0) & (s < 1e300)
                    L[:, i, i] = np.sqrt(np.where(ok, s, 1.0))
                else:
                    L[:, i, j] = s / L[:, j, j]
        for j in range(5):
            X = np.zeros((n, 5))
            X[:, j] = 1.0 / L[:, j, j]
            acc = X[:, j] * X[:, j]
            for i in range(j + 1, 5):
                s = np.zeros(n)
                for k in range(j, i):
                    s = s - L[:, i, k] * X[:, k]
                X[:, i] = s / L[:, i, i]
                acc = acc + X[:, i] * X[:, i]
            v[:, j] = acc
    return v, ok


def _check_mle_args(shape, gain, offset, read_var, sigma0, xtol):
    if len(shape) != 3 or shape[1] != shape[2]:
        raise ValueError(f"patches must be [N, P, P], got {tuple(shape)}")
    P = shape[1]
    if P % 2 != 1 or not 3 <= P <= 15:
        raise ValueError(f"patch side must be odd and from 3 to 15, got {P}")
    if not (gain > 0 and math.isfinite(gain)):
        raise ValueError(f"gain must be finite and > 0, got {gain}")
    if not math.isfinite(offset):
        raise ValueError(f"offset must be finite, got {offset}")
    if not (read_var >= 0 and math.isfinite(read_var)):
        raise ValueError(f"read_var must be finite and >= 0, got {read_var}")
    if not MLE_MIN_SIGMA < sigma0 < P:
        raise ValueError(f"sigma0 must lie in ({MLE_MIN_SIGMA}, {P}), got {sigma0}")
    if not 0 < xtol <= 1.49012e-8:
        raise ValueError(f"xtol must be in (0, 1.49012e-8], got {xtol}")


def _fit_mle_numpy(patches, gain=1.0, offset=0.0, read_var=0.0, sigma0=1.0, fit_sigma=True, xtol=FIT_XTOL,
                   max_iter=FIT_MAX_ITER):
    """The fit of csrc/localize.hip::ml_kernel for patches [N, P, P] on the host, all patches side by side -> (params [N, 5]
    float64 (photons, x0, y0, sigma, background), crlb [N, 5] float64, deviance [N] float64, status [N] int32, iterations
    [N] int32).  Equal to the kernel apart from erf, exp and log."""
    raw = np.asarray(patches)
    N, P, _ = raw.shape
    fs = bool(fit_sigma)
    status, iters = np.full(N, 2, np.int32), np.zeros(N, np.int32)
    crlb = np.full((N, 5), np.nan)
    if N == 0:
        return np.zeros((0, 5)), crlb, np.zeros(0), status, iters
    d = _mle_data(raw, gain, offset, read_var)
    flat = d.reshape(N, -1)
    finite = np.isfinite(raw.reshape(N, -1)).all(axis=1)
    mx, mn = flat.max(axis=1), flat.min(axis=1)
    total = np.zeros(N)
    for t in range(P * P):
        total = total + flat[:, t]
    with np.errstate(invalid="ignore"):
        b0 = np.maximum(mn, 1e-3 * mx)
        total = total - float(P * P) * b0
    p = np.stack([np.maximum(total, mx), np.full(N, float(P // 2)), np.full(N, float(P // 2)), np.full(N, float(sigma0)), b0],
                 axis=1)
    p[~finite] = np.nan
    cost, g, A, bad, mag = _mle_normal(d, p, read_var, fs)
    status[bad] = 1
    with np.errstate(invalid="ignore"):
        status[~bad & ~(cost < 1e300)] = 3
    status[~finite] = 3
    cost[~finite] = np.nan
    lam = np.full(N, 1e-3)
    for _ in range(max_iter):
        act = np.nonzero(status == 2)[0]
        if len(act) == 0:
            break
        iters[act] += 1
        dstep, ok = _fit_solve(A[act], g[act], lam[act])
        fail = act[~ok]
        lam[fail] *= 10.0
        status[fail[lam[fail] > 1e10]] = 1
        act, dstep = act[ok], dstep[ok]
        if len(act) == 0:
            continue
        pa = p[act]
        a0, a4 = np.abs(pa[:, 0]), np.abs(pa[:, 4])
        scale = np.stack([a0, np.maximum(np.abs(pa[:, 1]), 1.0), np.maximum(np.abs(pa[:, 2]), 1.0), np.abs(pa[:, 3]),
                          np.maximum(a4, a0)], axis=1)
        d0, ok0 = _fit_solve(A[act], g[act], 0.0)
        with np.errstate(invalid="ignore"):
            small = ok0 & (np.abs(d0) <= xtol * scale).all(axis=1)
        q = pa + dstep
        cq, gq, Aq, badq, mq = _mle_normal(d[act], q, read_var, fs)
        # the slack of the least-squares loop, taken of the magnitude of the summed terms: the deviance is a sum of differences
        # far larger than itself, and its rounding error is relative to those (csrc/spot_fit.h::sf_damped_fit)
        with np.errstate(invalid="ignore"):
            better = ~badq & (cq <= cost[act] + MLE_COST_SLACK * mag[act])
        up = act[better]
        p[up], cost[up], mag[up], g[up], A[up] = q[better], cq[better], mq[better], gq[better], Aq[better]
        lam[up] = np.maximum(lam[up] * 0.1, 1e-12)
        down = act[~better]
        lam[down] *= 10.0
        status[down[lam[down] > 1e10]] = 1
        status[act[small]] = 0
    done = np.nonzero(status == 0)[0]
    if len(done):
        v, ok = _mle_crlb(A[done])
        if not fs:
            v[:, 3] = 0.0
        crlb[done[ok]] = v[ok]
    return p, crlb, cost, status, iters


def fit_spots_mle(patches, gain=1.0, offset=0.0, read_var=0.0, sigma0=1.0, fit_sigma=True, xtol=FIT_XTOL):
    """Poisson maximum-likelihood fit of patches [N, P, P] (P odd, 3 .. 15; camera units, photons = max((patch - offset) /
    gain, 0), read_var the readout variance in photons^2) with the Cramer-Rao bound of every parameter: CUDA float tensors go
    to the kernel (ops.fit_spots_mle), anything else to the host restatement -> (params [N, 5] float64 (photons, x0, y0,
    sigma, background per pixel), crlb [N, 5] float64 (variances; NaN where status != 0), deviance [N] float64, status [N]
    int32, iterations [N] int32) of the input's kind.  fit_sigma=False holds sigma at sigma0."""
    gain, offset, read_var, sigma0, xtol = float(gain), float(offset), float(read_var), float(sigma0), float(xtol)
    _check_mle_args(patches.shape, gain, offset, read_var, sigma0, xtol)
    if _is_cuda(patches):
        from .. import ops
        return ops.fit_spots_mle(patches.float(), gain, offset, read_var, sigma0, bool(fit_sigma), xtol)
    if torch.is_tensor(patches):
        out = _fit_mle_numpy(patches.detach().numpy(), gain, offset, read_var, sigma0, fit_sigma, xtol)
        return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)
    return _fit_mle_numpy(patches, gain, offset, read_var, sigma0, fit_sigma, xtol)


# ----------------------------------------------------------------------------------------------------------------------
# joint fit of a localisation and its nearest neighbour (csrc/localize2.hip)
# ----------------------------------------------------------------------------------------------------------------------
_MLE2_ROW = np.array([i for i in range(8) for j in range(i + 1)])        # lower triangle row by row, as the kernel's lanes
_MLE2_COL = np.array([j for i in range(8) for j in range(i + 1)])


def _mle2_outside(p, P, two):
    """m2_outside: an N_e <= 0, s outside (MLE_MIN_SIGMA, P) or a centre outside [-1, P], of the live emitters."""
    with np.errstate(invalid="ignore"):
        bad = ~(p[:, 0] > 0.0) | ~(p[:, 6] > MLE_MIN_SIGMA) | ~(p[:, 6] < float(P))
        bad2 = ~(p[:, 3] > 0.0)
        for k in (1, 2):
            bad |= ~(p[:, k] >= -1.0) | ~(p[:, k] <= float(P))
            bad2 |= ~(p[:, 3 + k] >= -1.0) | ~(p[:, 3 + k] <= float(P))
    return bad | (two & bad2)


def _mle2_normal(d, p, two, read_var, fs):
    """Deviance, gradient [n, 8], Fisher matrix [n, 8, 8] (lower triangle), the out-of-domain flag and 2 sum(mu + d) of the
    two-emitter model at p [n, 8] = (N1, x1, y1, N2, x2, y2, s, b) for data d [n, P, P] in photons; two [n]: the rows with a
    second emitter (elsewhere N2 = x2 = y2 = 0 in p).  m2_eval of csrc/localize2.hip: the per-pixel quantities by the same
    expressions, every sum over the pixels in pixel order."""
    n, P, _ = d.shape
    with np.errstate(all="ignore"):
        bad = _mle2_outside(p, P, two)
        ok = ~bad
        q = np.where(ok[:, None], p, np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0]))   # placeholders: zeroed below
        Ex1, dEx1, sEx1 = (a.T[:, None, :] for a in _mle_axis(P, q[:, 1], q[:, 6], fs))     # [n, 1, P]
        Ey1, dEy1, sEy1 = (a.T[:, :, None] for a in _mle_axis(P, q[:, 2], q[:, 6], fs))     # [n, P, 1]
        Ex2, dEx2, sEx2 = (a.T[:, None, :] for a in _mle_axis(P, q[:, 4], q[:, 6], fs))
        Ey2, dEy2, sEy2 = (a.T[:, :, None] for a in _mle_axis(P, q[:, 5], q[:, 6], fs))
        N1, N2, t3 = q[:, 0, None, None], q[:, 3, None, None], two[:, None, None]
        nEy1, ndEy1, nsEy1 = N1 * Ey1, N1 * dEy1, N1 * sEy1
        nEy2, ndEy2, nsEy2 = N2 * Ey2, N2 * dEy2, N2 * sEy2
        mu = q[:, 7, None, None] + nEy1 * Ex1
        mu = np.where(t3, mu + nEy2 * Ex2, mu) + read_var
        J6 = nEy1 * sEx1 + nsEy1 * Ex1
        J6 = np.where(t3, J6 + (nEy2 * sEx2 + nsEy2 * Ex2), J6)
        zero = np.zeros_like(mu)
        J = np.stack([Ex1 * Ey1, nEy1 * dEx1, ndEy1 * Ex1, np.where(t3, Ex2 * Ey2, zero), np.where(t3, nEy2 * dEx2, zero),
                      np.where(t3, ndEy2 * Ex2, zero), J6, np.ones_like(mu)]).reshape(8, n, P * P)
        nonpos = (~(mu > 0.0)).reshape(n, -1).any(axis=1)
        rm = (1.0 / mu).reshape(n, -1)
        dd = d.reshape(n, -1)
        mu = mu.reshape(n, -1)
        r = dd * rm
        term = np.where(dd > 0.0, (mu - dd) + dd * np.log(np.where(dd > 0.0, r, 1.0)), mu)
        w = 1.0 - r
        tri, g, cost, mag = np.zeros((36, n)), np.zeros((8, n)), np.zeros(n), np.zeros(n)
        for t in range(P * P):                                                    # pixel order, one sum per entry
            Jt = J[:, :, t]
            tri = tri + (Jt[_MLE2_ROW] * rm[:, t]) * Jt[_MLE2_COL]
            g = g + Jt * w[:, t]
            cost = cost + term[:, t]
            mag = mag + (mu[:, t] + dd[:, t])
        cost, mag = 2.0 * cost, 2.0 * mag
        A = np.zeros((n, 8, 8))
        A[:, _MLE2_ROW, _MLE2_COL] = tri.T
        if not fs:
            A[:, 6, 6] = 1.0
        for k in (3, 4, 5):
            A[~two, k, k] = 1.0
        g = np.ascontiguousarray(g.T)
        cost[bad], mag[bad], g[bad], A[bad] = 0.0, 0.0, 0.0, 0.0
    return cost, g, A, bad | (ok & nonpos), mag


def _mle2_chol(A, lam):
    """Cholesky factor of A + lam diag(A) for every patch (csrc/spot_fit.h::sf_chol<8>) -> (L [n, 8, 8], ok [n])."""
    n = len(A)
    L = np.zeros((n, 8, 8))
    ok = np.ones(n, bool)
    for i in range(8):
        for j in range(i + 1):
            s = A[:, i, j].copy()
            if i == j:
                s = s + lam * s
            for k in range(j):
                s = s - L[:, i, k] * L[:, j, k]
            if i == j:
                ok &= (s > 0.0) & (s < 1e300)
                L[:, i, i] = np.sqrt(np.where(ok, s, 1.0))
            else:
                L[:, i, j] = s / L[:, j, j]
    return L, ok


def _mle2_solve(A, g, lam):
    """(A + lam diag(A)) d = -g by Cholesky for every patch (csrc/spot_fit.h::sf_solve<8>) -> (d [n, 8], ok [n])."""
    n = len(g)
    with np.errstate(all="ignore"):
        L, ok = _mle2_chol(A, lam)
        z = np.zeros((n, 8))
        for i in range(8):
            s = -g[:, i]
            for k in range(i):
                s = s - L[:, i, k] * z[:, k]
            z[:, i] = s / L[:, i, i]
        d = np.zeros((n, 8))
        for i in range(7, -1, -1):
            s = z[:, i]
            for k in range(i + 1, 8):
                s = s - L[:, k, i] * d[:, k]
            d[:, i] = s / L[:, i, i]
    return d, ok


def _mle2_crlb(A):
    """Diagonal of A^-1 through the Cholesky factor (csrc/spot_fit.h::sf_crlb<8>) -> (variances [n, 8], ok [n])."""
    n = len(A)
    v = np.zeros((n, 8))
    with np.errstate(all="ignore"):
        L, ok = _mle2_chol(A, 0.0)
        for j in range(8):
            X = np.zeros((n, 8))
            X[:, j] = 1.0 / L[:, j, j]
            acc = X[:, j] * X[:, j]
            for i in range(j + 1, 8):
                s = np.zeros(n)
                for k in range(j, i):
                    s = s - L[:, i, k] * X[:, k]
                X[:, i] = s / L[:, i, i]
                acc = acc + X[:, i] * X[:, i]
            v[:, j] = acc
    return v, ok


def _fit_mle2_numpy(patches, count, guess, gain=1.0, offset=0.0, read_var=0.0, sigma0=1.0, fit_sigma=True, xtol=FIT_XTOL,
                    max_iter=FIT_MAX_ITER):
    """The fit of csrc/localize2.hip::ml2_kernel for patches [N, P, P], count [N] and guess [N, 4] on the host, all patches
    side by side -> (params [N, 8] float64 (N1, x1, y1, N2, x2, y2, sigma, background), crlb [N, 8] float64, deviance [N]
    float64, status [N] int32, iterations [N] int32); the entries of emitter 2 are NaN where count = 1.  Equal to the kernel
    apart from erf, exp and log."""
    raw = np.asarray(patches)
    count, guess = np.asarray(count), np.asarray(guess, dtype=np.float64)
    N, P, _ = raw.shape
    fs = bool(fit_sigma)
    status, iters = np.full(N, 2, np.int32), np.zeros(N, np.int32)
    crlb = np.full((N, 8), np.nan)
    if N == 0:
        return np.zeros((0, 8)), crlb, np.zeros(0), status, iters
    two = count == 2
    d = _mle_data(raw, gain, offset, read_var)
    flat = d.reshape(N, -1)
    finite = np.isfinite(raw.reshape(N, -1)).all(axis=1) & (two | (count == 1))
    finite &= np.isfinite(guess[:, :2]).all(axis=1) & (~two | np.isfinite(guess[:, 2:]).all(axis=1))
    mx, mn = flat.max(axis=1), flat.min(axis=1)
    total = np.zeros(N)
    for t in range(P * P):
        total = total + flat[:, t]
    with np.errstate(invalid="ignore"):
        b0 = np.maximum(mn, 1e-3 * mx)
        total = total - float(P * P) * b0
        n0 = np.maximum(total, mx)
    zero = np.zeros(N)
    p = np.stack([np.where(two, 0.5 * n0, n0), guess[:, 0], guess[:, 1], np.where(two, 0.5 * n0, zero),
                  np.where(two, guess[:, 2], zero), np.where(two, guess[:, 3], zero), np.full(N, float(sigma0)), b0], axis=1)
    p[~finite] = np.nan
    cost, g, A, bad, mag = _mle2_normal(d, p, two, read_var, fs)
    with np.errstate(invalid="ignore"):
        same = two & ~_mle2_outside(p, P, two) & (p[:, 1] == p[:, 4]) & (p[:, 2] == p[:, 5])
    cost[same] = 0.0                           # two guesses on one point: a singular start, not evaluated (ml2_kernel)
    bad = bad | same
    status[bad] = 1
    with np.errstate(invalid="ignore"):
        status[~bad & ~(cost < 1e300)] = 3
    status[~finite] = 3
    cost[~finite] = np.nan
    lam = np.full(N, 1e-3)
    for _ in range(max_iter):
        act = np.nonzero(status == 2)[0]
        if len(act) == 0:
            break
        iters[act] += 1
        dstep, ok = _mle2_solve(A[act], g[act], lam[act])
        fail = act[~ok]
        lam[fail] *= 10.0
        status[fail[lam[fail] > 1e10]] = 1
        act, dstep = act[ok], dstep[ok]
        if len(act) == 0:
            continue
        pa = np.abs(p[act])
        a0 = np.maximum(pa[:, 0], pa[:, 3])
        scale = np.stack([pa[:, 0], np.maximum(pa[:, 1], 1.0), np.maximum(pa[:, 2], 1.0), pa[:, 3], np.maximum(pa[:, 4], 1.0),
                          np.maximum(pa[:, 5], 1.0), pa[:, 6], np.maximum(pa[:, 7], a0)], axis=1)
        d0, ok0 = _mle2_solve(A[act], g[act], 0.0)
        with np.errstate(invalid="ignore"):
            small = ok0 & (np.abs(d0) <= xtol * scale).all(axis=1)
        q = p[act] + dstep
        cq, gq, Aq, badq, mq = _mle2_normal(d[act], q, two[act], read_var, fs)
        with np.errstate(invalid="ignore"):
            better = ~badq & (cq <= cost[act] + MLE_COST_SLACK * mag[act])
        up = act[better]
        p[up], cost[up], mag[up], g[up], A[up] = q[better], cq[better], mq[better], gq[better], Aq[better]
        lam[up] = np.maximum(lam[up] * 0.1, 1e-12)
        down = act[~better]
        lam[down] *= 10.0
        status[down[lam[down] > 1e10]] = 1
        status[act[small]] = 0
    done = np.nonzero(status == 0)[0]
    if len(done):
        v, ok = _mle2_crlb(A[done])
        if not fs:
            v[:, 6] = 0.0
        crlb[done[ok]] = v[ok]
    one = np.nonzero(~two)[0]
    p[one[:, None], [3, 4, 5]] = np.nan
    crlb[one[:, None], [3, 4, 5]] = np.nan
    return p, crlb, cost, status, iters


def fit_spots_mle2(patches, count, guess, gain=1.0, offset=0.0, read_var=0.0, sigma0=1.0, fit_sigma=True, xtol=FIT_XTOL):
    """Joint Poisson maximum-likelihood fit of one or two emitters per patch with one width and one background: patches
    [N, P, P] and the camera model as fit_spots_mle, count [N] (1 or 2 emitters), guess [N, 4] (the starting centres x1, y1,
    x2, y2 in patch coordinates; the last two are ignored where count = 1).  CUDA float tensors go to the kernel
    (ops.fit_spots_mle2, csrc/localize2.hip), anything else to the host restatement -> (params [N, 8] float64 (N1, x1, y1, N2,
    x2, y2, sigma, background), crlb [N, 8] float64 (variances; NaN where status != 0), deviance [N] float64, status [N]
    int32, iterations [N] int32) of the input's kind.  Where count = 1 the fit is the five-parameter one and the entries of
    emitter 2 are NaN.  Two guesses on one point are a singular start (status 1, no iteration); two emitters that collapse
    onto each other on the way end with a non-zero status when the factor fails."""
    gain, offset, read_var, sigma0, xtol = float(gain), float(offset), float(read_var), float(sigma0), float(xtol)
    _check_mle_args(patches.shape, gain, offset, read_var, sigma0, xtol)
    n = patches.shape[0]
    if tuple(count.shape) != (n,) or tuple(guess.shape) != (n, 4):
        raise ValueError(f"count must be [{n}] and guess [{n}, 4], got {tuple(count.shape)} and {tuple(guess.shape)}")
    cuda = _is_cuda(patches)
    cnt = torch.as_tensor(count).to(patches.device) if cuda else torch.as_tensor(np.asarray(count))
    gs = torch.as_tensor(guess).to(patches.device) if cuda else torch.as_tensor(np.asarray(guess))
    if cnt.is_floating_point() or cnt.dtype == torch.bool or not bool(((cnt == 1) | (cnt == 2)).all()):
        raise ValueError("count must hold integers 1 or 2")
    gs = gs.double()
    if not bool((torch.isfinite(gs[:, :2]).all(dim=1) & ((cnt == 1) | torch.isfinite(gs[:, 2:]).all(dim=1))).all()):
        raise ValueError("guess must be finite (the last two columns where count = 2)")
    if cuda:
        from .. import ops
        return ops.fit_spots_mle2(patches.float(), cnt.int(), gs, gain, offset, read_var, sigma0, bool(fit_sigma), xtol)
    host = patches.detach().numpy() if torch.is_tensor(patches) else patches
    out = _fit_mle2_numpy(host, cnt.numpy(), gs.numpy(), gain, offset, read_var, sigma0, fit_sigma, xtol)
    if torch.is_tensor(patches):
        return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)
    return out


def _spot_neighbours_numpy(frame_offsets, ys, xs, reach):
    """nb_kernel of csrc/localize2.hip on the host: rows sorted by frame -> (neighbour [n], n_neighbours [n]) int32."""
    off, ys, xs = np.asarray(frame_offsets, np.int64), np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    n = len(ys)
    neighbour, within = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for f in range(len(off) - 1):
        a, b = max(int(off[f]), 0), min(int(off[f + 1]), n)
        if b - a < 2:
            continue
        dy, dx = np.abs(ys[a:b, None] - ys[None, a:b]), np.abs(xs[a:b, None] - xs[None, a:b])
        ok = (dy <= reach) & (dx <= reach)
        np.fill_diagonal(ok, False)
        d2 = np.where(ok, dy * dy + dx * dx, np.iinfo(np.int64).max)
        neighbour[a:b] = np.where(ok.any(axis=1), a + np.argmin(d2, axis=1), -1)       # argmin: the first, so the lower row
        within[a:b] = ok.sum(axis=1)
    return neighbour, within


def spot_neighbours(frames, ys, xs, reach):
    """For every localisation the nearest other one of its frame within a square reach: frames / ys / xs [n] in any order
    (positions are rounded half-to-even, as extract_patches_flat cuts its patches) -> (neighbour [n] int64: the row, in the
    caller's order, with max(|dy|, |dx|) <= reach that is nearest by squared Euclidean distance, ties to the lower row, -1 if
    there is none; n_neighbours [n] int64: the rows within reach) of the input's kind.  CUDA tensors: a stable sort by frame
    and the CSR over it with torch ops, then ops.spot_neighbours (csrc/localize2.hip); anything else the same on the host."""
    if int(reach) != reach or reach < 0:
        raise ValueError(f"reach must be an integer >= 0, got {reach}")
    if not (len(frames) == len(ys) == len(xs)):
        raise ValueError("frames, ys and xs must have one entry per localisation")
    n = len(frames)
    if _is_cuda(frames) and _is_cuda(ys) and _is_cuda(xs):
        from .. import ops
        dev = frames.device
        fr = frames.long()
        if n == 0:
            return torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
        if int(fr.min()) < 0:
            raise ValueError("frames must be >= 0")
        fs, order = torch.sort(fr, stable=True)
        offsets = torch.zeros(int(fs[-1]) + 2, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(torch.bincount(fs), 0)
        yy, xx = torch.round(ys.double()).int()[order], torch.round(xs.double()).int()[order]
        nb, within = ops.spot_neighbours(offsets.int(), yy.contiguous(), xx.contiguous(), int(reach))
        neighbour = torch.empty(n, dtype=torch.int64, device=dev)
        neighbour[order] = torch.where(nb >= 0, order[nb.long().clamp(min=0)], torch.full_like(order, -1))
        count = torch.empty(n, dtype=torch.int64, device=dev)
        count[order] = within.long()
        return neighbour, count
    is_t = torch.is_tensor(frames)
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    fr = host(frames).astype(np.int64)
    if n and fr.min() < 0:
        raise ValueError("frames must be >= 0")
    order = np.argsort(fr, kind="stable")
    offsets = np.zeros(int(fr.max()) + 2 if n else 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(fr)) if n else 0
    yy = np.rint(host(ys).astype(np.float64)).astype(np.int64)[order]
    xx = np.rint(host(xs).astype(np.float64)).astype(np.int64)[order]
    nb, within = _spot_neighbours_numpy(offsets, yy, xx, int(reach))
    neighbour, count = np.empty(n, np.int64), np.empty(n, np.int64)
    neighbour[order] = np.where(nb >= 0, order[np.maximum(nb, 0)], -1)
    count[order] = within
    if is_t:
        return torch.from_numpy(neighbour), torch.from_numpy(count)
    return neighbour, count


def _check_neighbours(neighbours, method, frames, P):
    """neighbours: None, True or {"reach": r} -> the reach, or None"""
    if neighbours is None or neighbours is False:
        return None
    if neighbours is not True and (not isinstance(neighbours, dict) or set(neighbours) - {"reach"}):
        raise ValueError("neighbours must be None, True or a dict with the key reach")
    if method != "mle":
        raise ValueError("neighbours needs method='mle': the joint fit is a maximum-likelihood fit")
    if frames is None:
        raise ValueError("neighbours needs frames: a neighbour is a localisation of the same frame")
    reach = P // 2 if neighbours is True else neighbours.get("reach", P // 2)
    if int(reach) != reach or not 0 <= reach <= P // 2 + 1:                  # the fit keeps a centre within [-1, P]
        raise ValueError(f"neighbours['reach'] must be an integer from 0 to P // 2 + 1 = {P // 2 + 1}, got {reach}")
    return int(reach)


def _fit_with_neighbours(patches, frames, ys, xs, reach, camera):
    """The joint fit of every row with its nearest neighbour (count = 1 where it has none), guessed at the patch centre and
    at the neighbour's offset from it -> (params [N, 8], crlb [N, 8], deviance, status, neighbour, n_neighbours): CUDA tensors
    for CUDA patches, numpy arrays otherwise."""
    half = patches.shape[1] // 2
    if len(frames) != len(patches) or len(ys) != len(patches) or len(xs) != len(patches):
        raise ValueError("patches, frames, ys and xs must have one entry per localisation")
    if _is_cuda(patches):
        dev = patches.device
        fr, yy, xx = (torch.as_tensor(a).to(dev) for a in (frames, ys, xs))
        yy, xx = torch.round(yy.double()), torch.round(xx.double())
        nb, within = spot_neighbours(fr, yy, xx, reach)
        has, j = nb >= 0, nb.clamp(min=0)
        centre, zero = torch.full_like(yy, float(half)), torch.zeros_like(yy)
        guess = torch.stack([centre, centre, torch.where(has, half + (xx[j] - xx), zero),
                             torch.where(has, half + (yy[j] - yy), zero)], dim=1)
        params, crlb, dev_, status, _ = fit_spots_mle2(patches, torch.where(has, 2, 1).int(), guess, **camera)
        return params, crlb, dev_, status, nb, within
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    yy, xx = np.rint(host(ys).astype(np.float64)), np.rint(host(xs).astype(np.float64))
    nb, within = spot_neighbours(host(frames), yy, xx, reach)
    has, j = nb >= 0, np.maximum(nb, 0)
    centre, zero = np.full(len(yy), float(half)), np.zeros(len(yy))
    guess = np.stack([centre, centre, np.where(has, half + (xx[j] - xx), zero), np.where(has, half + (yy[j] - yy), zero)],
                     axis=1)
    params, crlb, dev_, status, _ = fit_spots_mle2(host(patches), np.where(has, 2, 1).astype(np.int32), guess, **camera)
    return params, crlb, dev_, status, nb, within


_PRIMARY = [0, 1, 2, 6, 7]      # (N1, x1, y1, sigma, background) of the joint fit: the columns of the single-emitter fit
_CAMERA_KEYS = ("gain", "offset", "read_var", "sigma0", "fit_sigma")


def _check_refine_method(method, camera):
    if method not in ("lsq", "mle"):
        raise ValueError(f"method must be 'lsq' or 'mle', got {method!r}")
    if camera is not None and (not isinstance(camera, dict) or set(camera) - set(_CAMERA_KEYS)):
        raise ValueError(f"camera must be None or a dict with keys among {', '.join(_CAMERA_KEYS)}")
    if camera is not None and method != "mle":
        raise ValueError("camera needs method='mle': the least-squares fit has no camera model")
    return dict(camera or {})


def refine_localizations(patches, ys, xs, method="lsq", camera=None, frames=None, neighbours=None):
    """Sub-pixel positions of N localisations without pandas: patches [N, P, P] (extract_patches_flat) around the integer
    positions ys / xs [N] -> dict of numpy arrays x_refined, y_refined, psf_size (float64), max_intensity (the patches' dtype)
    and status (int32).  Where the fit failed (status != 0) the reference's fallback applies: the integer position and
    psf_size 10.

    method "lsq" (default: the reference's unweighted least-squares fit, the code path without the argument) or "mle": the
    Poisson maximum-likelihood fit (fit_spots_mle) with the camera model `camera`, a dict with keys among gain, offset,
    read_var, sigma0 and fit_sigma.  "mle" adds x_std, y_std (square roots of the Cramer-Rao bounds, pixels), photons,
    background (photons per pixel) and deviance (float64); they are NaN where status != 0.

    neighbours (default None: every localisation fitted alone, the code path without the argument): True or {"reach": r}, with
    method "mle" and frames [N], the frame of every row.  Each row learns its nearest neighbour of the same frame inside its
    patch (spot_neighbours; r from 0 to P // 2 + 1, the last pixel the fit lets a centre reach; default P // 2) and is fitted jointly with it (fit_spots_mle2, csrc/localize2.hip:
    one width and one background for both, the row's own centre guessed at the patch centre, the neighbour's at its offset);
    a row without one goes through the same fit with one emitter.  The keys above carry the row's own emitter; the result
    gains n_neighbours (int64, the rows within reach: with more than one the fit is with the nearest), neighbour (int64,
    its row or -1) and photons_neighbour (float64, NaN without a neighbour or where status != 0)."""
    camera = _check_refine_method(method, camera)
    reach = _check_neighbours(neighbours, method, frames, patches.shape[1])
    if reach is not None:
        tonp = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        params8, crlb8, dev, status, nb, within = (tonp(t) for t in _fit_with_neighbours(patches, frames, ys, xs, reach, camera))
        params, crlb = params8[:, _PRIMARY], crlb8[:, _PRIMARY]
        flat = tonp(patches).reshape(len(patches), -1)
        peak = flat.max(axis=1) if len(flat) else flat[:, 0]
    elif method == "mle":
        params, crlb, dev, status, _ = fit_spots_mle(patches, **camera)
        flat = patches.reshape(len(patches), -1)
        if torch.is_tensor(params):
            params, crlb, dev, status = (t.cpu().numpy() for t in (params, crlb, dev, status))
            flat = flat.cpu().numpy()
        peak = flat.max(axis=1) if len(flat) else flat[:, 0]
    else:
        params, peak, status = refine_gaussian_patches(patches)
        if torch.is_tensor(params):
            params, peak, status = params.cpu().numpy(), peak.cpu().numpy(), status.cpu().numpy()
    half = patches.shape[1] // 2
    if _is_cuda(ys):
        ys, xs = ys.cpu(), xs.cpu()
    ys, xs = np.asarray(ys), np.asarray(xs)
    okf = status == 0
    res = {"x_refined": np.where(okf, xs - half + params[:, 1], xs.astype(np.float64)),
           "y_refined": np.where(okf, ys - half + params[:, 2], ys.astype(np.float64)),
           "psf_size": np.where(okf, params[:, 3], float(FALLBACK_PSF_SIZE)),
           "max_intensity": peak, "status": status}
    if method == "mle":
        with np.errstate(invalid="ignore"):
            res.update({"x_std": np.sqrt(crlb[:, 1]), "y_std": np.sqrt(crlb[:, 2]),
                        "photons": np.where(okf, params[:, 0], np.nan), "background": np.where(okf, params[:, 4], np.nan),
                        "deviance": np.where(okf, dev, np.nan)})
    if reach is not None:
        res.update({"n_neighbours": within, "neighbour": nb, "photons_neighbour": np.where(okf, params8[:, 3], np.nan)})
    return res


def add_refined_localization_to_dataframe(df_tracks, tracks, patches, patch_size):
    """Reference add_refined_localization_to_dataframe: adds x_refined, y_refined, psf_size and max_intensity to a DataFrame
    indexed by (track_id, frame).  All patches of all tracks are fitted in one call."""
    import pandas as pd
    keys, ys, xs, stack = [], [], [], []
    for tid, positions in tracks.items():
        tp = patches[tid]
        for i, (frame, y, x) in enumerate(positions):
            keys.append((tid, frame))
            ys.append(y)
            xs.append(x)
            stack.append(tp[i])
    if not keys:
        for col in ("x_refined", "y_refined", "psf_size", "max_intensity"):
            df_tracks[col] = pd.Series(dtype=np.float64)
        return df_tracks
    allp = torch.stack(stack) if torch.is_tensor(stack[0]) else np.stack(stack)
    if allp.shape[1] != patch_size:
        raise ValueError(f"patches of side {allp.shape[1]} with patch_size = {patch_size}")
    res = refine_localizations(allp, np.asarray(ys), np.asarray(xs))
    for col in ("x_refined", "y_refined", "psf_size", "max_intensity"):
        df_tracks[col] = pd.Series(dict(zip(keys, res[col])))
    return df_tracks


def compute_displacement(df_tracks):
    """Reference compute_displacement: per-step displacement of the refined positions (0 at a track's first frame) and the
    per-track columns mean_displacement, mean_psf_size, max_intensity_over_track, mean_max_intensity_over_track,
    std_max_intensity_over_track."""
    df = df_tracks.reset_index()
    per_track = {k: {} for k in ("mean_displacement", "mean_psf_size", "max_intensity_over_track",
                                 "mean_max_intensity_over_track", "std_max_intensity_over_track")}
    for tid, group in df.groupby("track_id"):
        group = group.sort_values("frame")
        x, y = group["x_refined"].to_numpy(), group["y_refined"].to_numpy()
        steps = [0] + list(np.sqrt((x[1:] - x[:-1]) ** 2 + (y[1:] - y[:-1]) ** 2))
        df.loc[group.index, "displacement"] = steps
        per_track["mean_displacement"][tid] = np.mean(steps)
        per_track["mean_psf_size"][tid] = group["psf_size"].mean()
        per_track["max_intensity_over_track"][tid] = group["max_intensity"].max()
        per_track["mean_max_intensity_over_track"][tid] = group["max_intensity"].mean()
        per_track["std_max_intensity_over_track"][tid] = group["max_intensity"].std()
    df.set_index(["track_id", "frame"], inplace=True)
    ids = df.index.get_level_values("track_id")
    for col, values in per_track.items():
        df[col] = ids.map(values)
    return df


def tracks_to_dataframe(tracks, patches, patch_size):
    """Reference tracks_to_dataframe: tracks {id: [(frame, y, x), ...]} and their patches -> DataFrame indexed by (track_id,
    frame) with nbr_frames, x, y, the refined localisation and the displacement columns."""
    import pandas as pd
    data = [(tid, frame, len(positions), x, y) for tid, positions in tracks.items() for frame, y, x in positions]
    df = pd.DataFrame(data, columns=["track_id", "frame", "nbr_frames", "x", "y"])
    df.set_index(["track_id", "frame"], inplace=True)
    df.sort_index(inplace=True)
    df = add_refined_localization_to_dataframe(df, tracks, patches, patch_size=patch_size)
    return compute_displacement(df)


# ----------------------------------------------------------------------------------------------------------------------
# from the table to one diffusion coefficient per track
# ----------------------------------------------------------------------------------------------------------------------
def tracks_table_by_track(table):
    """The dict track_particles_tensors returns -> (frame, y, x, track_id [N'] int64, offsets [n_tracks + 1] int64), tensors on
    the table's device: the rows with in_long_track, stably sorted by track_id (the table is in frame order, so every track
    stays in frame order), and the CSR offsets of the tracks in ascending id.  A table with the column filled
    (track_particles_tensors(..., max_gap > 0)) returns a sixth tensor, filled [N'] bool, in the same row order."""
    keep = torch.as_tensor(table["in_long_track"]).bool()
    if "filled" in table:
        fr, y, x, tid, offsets = tracks_table_by_track({k: v for k, v in table.items() if k != "filled"})
        filled = torch.as_tensor(table["filled"]).to(keep.device)
        if filled.shape != keep.shape:
            raise ValueError("filled must have one entry per row")
        filled = filled[keep]
        return fr, y, x, tid, offsets, filled[torch.argsort(torch.as_tensor(table["track_id"]).to(keep.device)[keep],
                                                            stable=True)].bool()
    cols = [torch.as_tensor(table[k]).to(keep.device)[keep] for k in ("frame", "y", "x", "track_id")]
    if not (len(cols[0]) == len(cols[1]) == len(cols[2]) == len(cols[3])):
        raise ValueError("frame, y, x and track_id must have one entry per row")
    order = torch.argsort(cols[3], stable=True)
    fr, y, x, tid = (c[order].long() for c in cols)
    _, counts = torch.unique_consecutive(tid, return_counts=True)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=tid.device), torch.cumsum(counts, 0)])
    return fr, y, x, tid, offsets


def _check_sequence_args(seq_len, tail, patch_size=None):
    if patch_size is not None and (int(patch_size) != patch_size or patch_size % 2 != 1 or not 3 <= patch_size <= 15):
        raise ValueError(f"patch_size must be an odd number from 3 to 15, got {patch_size}")
    if int(seq_len) != seq_len or seq_len < 1:
        raise ValueError(f"seq_len must be an integer >= 1, got {seq_len}")
    if tail not in ("drop", "overlap"):
        raise ValueError(f"tail must be 'drop' or 'overlap', got {tail!r}")


def _check_csr(offsets, n=None):
    if len(offsets.shape) != 1 or offsets.shape[0] < 1:
        raise ValueError(f"offsets must be [n_tracks + 1], got {tuple(offsets.shape)}")
    first, last = int(offsets[0]), int(offsets[-1])
    if first != 0 or (n is not None and last != n):
        raise ValueError(f"offsets must start at 0 and end at the number of rows{'' if n is None else f' {n}'}, "
                         f"got {first} .. {last}")
    if offsets.shape[0] > 1 and bool((offsets[1:] < offsets[:-1]).any()):
        raise ValueError("offsets must not decrease")


def plan_sequences(offsets, seq_len, tail="drop"):
    """Windows of seq_len consecutive rows per track: offsets [n_tracks + 1] (CSR, array or tensor) -> (seq_row [n_seq], the
    table row where each window starts, seq_track [n_seq], the index of its track), int64, of the input's kind and device.
    Per track of L rows L // seq_len windows side by side from the track's start; tail="drop" leaves the remaining rows out,
    tail="overlap" adds one window aligned to the track's end when L % seq_len != 0 and L >= seq_len (it overlaps the one
    before).  A track shorter than seq_len gives no window.  The windows of a track are contiguous in the output and in
    ascending row, tracks in ascending order.  No loop over the tracks."""
    _check_sequence_args(seq_len, tail)
    is_t = torch.is_tensor(offsets)
    off = offsets.long() if is_t else np.asarray(offsets).astype(np.int64)
    _check_csr(off)
    T = int(seq_len)
    lengths = off[1:] - off[:-1]
    n_full = lengths // T
    n_win = n_full
    if tail == "overlap":
        extra = (lengths % T != 0) & (lengths >= T)
        n_win = n_full + (extra.long() if is_t else extra.astype(np.int64))
    first = (torch.cumsum(n_win, 0) if is_t else np.cumsum(n_win)) - n_win
    if is_t:
        seq_track = torch.repeat_interleave(torch.arange(len(lengths), device=off.device), n_win)
        j = torch.arange(len(seq_track), device=off.device) - first[seq_track]
        where = torch.where
    else:
        seq_track = np.repeat(np.arange(len(lengths), dtype=np.int64), n_win)
        j = np.arange(len(seq_track), dtype=np.int64) - first[seq_track]
        where = np.where
    seq_row = off[:-1][seq_track] + where(j < n_full[seq_track], j * T, lengths[seq_track] - T)
    return seq_row, seq_track


def _rounded_int32(v, device):
    """Positions rounded half-to-even as extract_patches_flat rounds them, as an int32 tensor on `device`."""
    if torch.is_tensor(v):
        v = v if not v.is_floating_point() else torch.round(v.double())
        return v.to(device=device, dtype=torch.int32)
    return torch.as_tensor(np.rint(np.asarray(v, dtype=np.float64)).astype(np.int32), device=device)


def track_sequences(movie, frames, ys, xs, offsets, seq_len, patch_size=7, norm=None, tail="drop"):
    """The normalised patch sequences a GeneralTransformer consumes, from the table sorted by track (tracks_table_by_track):
    movie [F, H, W] float32, frames / ys / xs [N], offsets [n_tracks + 1] -> (seq [n_seq, seq_len, patch_size, patch_size]
    float32, seq_track [n_seq], seq_row [n_seq]); the windows are plan_sequences(offsets, seq_len, tail).  The patch of step t
    of window s is centred on the position of row seq_row[s] + t, rounded half-to-even; pixels outside the frame read as 0.
    norm = (background_mean, background_sigma, theoretical_max) as helpers/generation.normalize_images takes them: every pixel
    (the zeros outside the frame included) becomes (v - lo) / denom with lo = background_mean - background_sigma and
    denom = theoretical_max - lo; norm=None returns the raw patches.  A row whose frame lies outside the movie gives a zero
    patch.  A CUDA movie goes to the kernel (ops.track_sequences, one launch) and returns CUDA tensors; anything else goes to
    extract_patches_flat and the same arithmetic in torch on the CPU, bitwise equal, and returns the movie's kind."""
    _check_sequence_args(seq_len, tail, patch_size)
    if len(movie.shape) != 3:
        raise ValueError(f"movie must be [F, H, W], got {tuple(movie.shape)}")
    if not (len(frames) == len(ys) == len(xs)):
        raise ValueError("frames, ys and xs must have one entry per row")
    _check_csr(offsets if torch.is_tensor(offsets) else np.asarray(offsets), len(frames))
    lo, denom = 0.0, 1.0
    if norm is not None:
        background_mean, background_sigma, theoretical_max = (float(v) for v in norm)
        lo = background_mean - background_sigma
        denom = theoretical_max - lo
        if denom == 0:
            raise ValueError("Denominator in normalization is zero. Check your inputs.")
    T, P = int(seq_len), int(patch_size)
    if _is_cuda(movie):
        from .. import ops
        dev = movie.device
        off = torch.as_tensor(offsets, device=dev)
        seq_row, seq_track = plan_sequences(off, T, tail)
        seq = ops.track_sequences(movie, torch.as_tensor(frames).to(dev, torch.int32), _rounded_int32(ys, dev),
                                  _rounded_int32(xs, dev), seq_row.int(), T, P, lo, denom, norm is not None)
        return seq, seq_track, seq_row
    is_np = not torch.is_tensor(movie)
    img = torch.as_tensor(np.asarray(movie)) if is_np else movie.detach()
    if img.dtype != torch.float32:
        raise TypeError(f"movie must be float32, got {img.dtype}")
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)      # noqa: E731
    seq_row, seq_track = plan_sequences(host(offsets), T, tail)
    rows = (seq_row[:, None] + np.arange(T, dtype=np.int64)[None, :]).reshape(-1)
    fr = host(frames).astype(np.int64)[rows]
    inside = (fr >= 0) & (fr < img.shape[0])
    patches = extract_patches_flat(img, np.where(inside, fr, 0), host(ys)[rows], host(xs)[rows], P)
    if norm is not None:
        patches = (patches - lo) / denom
    patches = torch.where(torch.from_numpy(inside)[:, None, None], patches, torch.zeros((), dtype=patches.dtype))
    seq = patches.reshape(len(seq_row), T, P, P)
    if is_np:
        return seq.numpy(), seq_track, seq_row
    return seq, torch.from_numpy(seq_track), torch.from_numpy(seq_row)


def refine_localizations_tensors(patches, ys, xs, method="lsq", camera=None, frames=None, neighbours=None):
    """refine_localizations without the copy to the host: CUDA patches [N, P, P] (extract_patches_flat) around the integer
    positions ys / xs [N] -> dict of CUDA tensors x_refined, y_refined, psf_size (float64), max_intensity (float32) and status
    (int32), with the same fallback where the fit failed (status != 0): the integer position and psf_size 10.  method and
    camera as refine_localizations: "mle" adds x_std, y_std, photons, background and deviance (float64, NaN where status !=
    0).  frames and neighbours as refine_localizations: the joint fit with the nearest neighbour of the same frame, which adds
    n_neighbours, neighbour (int64) and photons_neighbour (float64)."""
    if not _is_cuda(patches):
        raise ValueError("refine_localizations_tensors needs CUDA patches; use refine_localizations on the host")
    camera = _check_refine_method(method, camera)
    reach = _check_neighbours(neighbours, method, frames, patches.shape[1])
    if reach is not None:
        params8, crlb8, dev, status, nb, within = _fit_with_neighbours(patches, frames, ys, xs, reach, camera)
        params, crlb = params8[:, _PRIMARY], crlb8[:, _PRIMARY]
        peak = patches.float().reshape(len(patches), -1).amax(dim=1) if len(patches) else patches.float().reshape(0)
    elif method == "mle":
        params, crlb, dev, status, _ = fit_spots_mle(patches, **camera)
        peak = patches.float().reshape(len(patches), -1).amax(dim=1) if len(patches) else patches.float().reshape(0)
    else:
        params, peak, status = refine_gaussian_patches(patches)
    half = patches.shape[1] // 2
    ys, xs = torch.as_tensor(ys).to(patches.device), torch.as_tensor(xs).to(patches.device)
    if not (len(ys) == len(xs) == len(params)):
        raise ValueError("patches, ys and xs must have one entry per localisation")
    okf = status == 0
    res = {"x_refined": torch.where(okf, xs - half + params[:, 1], xs.double()),
           "y_refined": torch.where(okf, ys - half + params[:, 2], ys.double()),
           "psf_size": torch.where(okf, params[:, 3], torch.full_like(params[:, 3], float(FALLBACK_PSF_SIZE))),
           "max_intensity": peak, "status": status}
    if method == "mle":
        nan = torch.full_like(dev, float("nan"))
        res.update({"x_std": torch.sqrt(crlb[:, 1]), "y_std": torch.sqrt(crlb[:, 2]),
                    "photons": torch.where(okf, params[:, 0], nan), "background": torch.where(okf, params[:, 4], nan),
                    "deviance": torch.where(okf, dev, nan)})
    if reach is not None:
        res.update({"n_neighbours": within, "neighbour": nb, "photons_neighbour": torch.where(okf, params8[:, 3], nan)})
    return res


_TRANSPORT_KEYS = ("min_len", "penalty", "velocity_penalty", "min_var", "classes", "blur")


def transport_per_track(seg_offsets, seg_track, seg_class, lengths):
    """What a track's stretches (helpers/msd.segment_transport: seg_offsets [n_seg + 1], seg_track, seg_class [n_seg]) say
    about the track as a whole, for tracks of lengths [n_tracks] rows; int64 tensors on one device -> (run_fraction [n_tracks]
    float64, the share of the track's rows that lie in directed stretches (NaN for a track without rows); n_runs [n_tracks]
    int64, its directed stretches)."""
    n_tracks = len(lengths)
    rows = (seg_offsets[1:] - seg_offsets[:-1]) * seg_class
    run_rows = torch.zeros(n_tracks, dtype=torch.int64, device=lengths.device).index_add_(0, seg_track, rows)
    n_runs = torch.zeros(n_tracks, dtype=torch.int64, device=lengths.device).index_add_(0, seg_track, seg_class)
    return run_rows.double() / lengths.double(), n_runs


def estimate_track_diffusion(movie, model, seq_len, patch_size=7, dt=1.0, norm=None, refine=True, tail="drop",
                             batch_size=4096, segment=None, states=None, drift=None, localization=None, ml=None, anomalous=None,
                             confined=None, directed=None, transport=None, **tracking_kwargs):
    """One diffusion coefficient per track of a CUDA movie [F, H, W], from a trained model and from the classical MSD estimate
    it is compared with, without leaving the device: track_particles_tensors(movie, **tracking_kwargs), tracks_table_by_track,
    (with refine) extract_patches_flat + refine_localizations_tensors, helpers/msd.track_msd on (y_refined, x_refined) -- on
    the integer positions with refine=False --, track_sequences(..., seq_len, patch_size, norm, tail), model.eval() under
    torch.no_grad() in chunks of batch_size sequences, and the mean of the model's first output column over the sequences of
    each track (float64, in sequence order: deterministic).  -> dict of CUDA tensors track_id, length, n_sequences (int64
    [n_tracks]), D_model (float64; NaN where n_sequences == 0), D_msd, D_msd_weighted (float64, in pixels^2 per unit of dt) and
    msd [n_tracks, longest track].  D_model is the model's output in the units it was trained in: no scale factor is applied
    here.  With max_gap > 0 among the tracking arguments the tracks are gap-closed and filled: length counts rows, the filled
    ones included, the result gains n_filled (int64 [n_tracks], the filled rows of each track), and with refine the filled
    rows are fitted on their patch like any other row (a failed fit falls back to the interpolated position).

    segment (default None: one number per track, the code path without it): a dict of helpers/msd.segment_tracks arguments
    (min_len, penalty, min_var, blur; {} for the defaults; dt is this function's).  The result gains "segments": the
    segment_tracks dict computed on the positions the MSD is taken on (csrc/segment.hip), plus D_model [n_seg], the mean of
    the model's output over the windows of plan_sequences(seg_offsets, seq_len, tail), so that no window straddles a
    changepoint (NaN for a segment shorter than seq_len), and n_sequences [n_seg].  The per-track entries are unchanged.

    states (default None: off): a dict of helpers/msd.fit_diffusion_states arguments (K, required; sigma2, max_iter, tol,
    min_var, init; dt is this function's).  The result gains "states": the fit_diffusion_states dict computed on the same
    positions (csrc/hmm.hip: diffusion states SHARED by all tracks, where segment cuts each track on its own), plus
    run_offsets [n_runs + 1], the CSR of the maximal runs of constant Viterbi state over the same rows (it refines offsets),
    run_track and run_state [n_runs] (-1 for a one-row track), and D_model, n_sequences [n_runs] from the windows of
    plan_sequences(run_offsets, seq_len, tail) exactly as for segment, so that no window straddles a switch.  The per-track
    entries and those of segment are unchanged; both may be given.

    drift (default None: a stage at rest, the code path without it): a dict of helpers/msd.estimate_drift arguments (estimator,
    smoothing, min_pairs; {} for the defaults).  The drift of the stage is estimated from the increments of all tracks on the
    positions the MSD is taken on (refined or integer; the filled rows of gap-closed tracks are left out of the estimate
    through use) and subtracted (csrc/drift.hip), and track_msd, segment and states run on the corrected positions.  The
    result gains "drift": the estimate_drift dict plus positions, the corrected [N, 2].  D_model is unchanged by
    construction: the patches are cut from the movie at the detected positions, and a patch does not know where the stage
    is.

    localization (default None: the least-squares refinement, the code path without it): a dict with keys among gain, offset,
    read_var, sigma0 and fit_sigma ({} for the defaults), the camera model of fit_spots_mle; needs refine=True.  The
    refinement is then the Poisson maximum-likelihood fit (csrc/localize.hip, refine_localizations_tensors(method="mle")), and
    the result gains "localization", the per-row tensors y_std, x_std (pixels), photons, background, psf_size, deviance and
    status in the row order of tracks_table_by_track, and sigma2_loc [n_tracks]: the mean of (y_std^2 + x_std^2) / 2 over a
    track's rows with status 0 that are not filled, NaN where there is none.  states = {"sigma2": "crlb", ...} passes the mean
    of that quantity over all such rows of the movie to fit_diffusion_states as its localisation variance and reports it as
    states["sigma2"] (the key is there only then); it is a ValueError without localization.  localization may also hold
    "neighbours": True or {"reach": r} (refine_localizations_tensors): every row is fitted jointly with its nearest neighbour of
    the same frame inside its patch (csrc/localize2.hip), the positions, "localization" and sigma2_loc come from the joint fit
    and its bounds, and "localization" gains n_neighbours, neighbour (rows of tracks_table_by_track) and photons_neighbour.

    detector (one of tracking_kwargs, default None: the difference of Gaussians): {"method": "lrt", ...}, the likelihood-ratio
    detector of track_particles_tensors; gain, offset, read_var and sigma0 it does not name are those of localization.

    ml (default None: the code path without it): a dict with keys among blur and sigma2 ({} for the defaults), the arguments of
    helpers/msd.estimate_diffusion_ml (csrc/likelihood.hip), the maximum-likelihood D of every track from rows of known
    variance, with a standard error.  blur is the motion-blur coefficient (default 0).  sigma2 is the localisation variance
    per coordinate: a number (default 0 without localization), with which every row that is not filled is used, or "crlb" (the
    default with localization; a ValueError without it, like states["sigma2"] = "crlb"): every row carries (y_std^2, x_std^2)
    of its own fit, and the rows used are those with status 0 that are not filled, the set sigma2_loc is taken over.  It
    runs on the positions the MSD is taken on (drift-corrected if drift is given) with the frames of the table, so a filled
    row is a gap of the likelihood, not an interpolated position.  The result gains D_ml, D_ml_std (float64) and ml_status
    (int64) [n_tracks], and "ml": what estimate_diffusion_ml was called with (positions [N, 2], variances [N, 2] or the
    number, frames [N], use [N] bool or None, blur).  With segment, "segments" gains D_ml, D_ml_std and ml_status per segment
    (the same call on seg_offsets), and with states, "states" gains them per run (on run_offsets).  segments["D_mle"] keeps
    its name and meaning: it is <q> / (4 dt), the maximum-likelihood estimate of a track WITHOUT localisation noise and blur,
    which noise biases upwards by sigma^2 / dt; D_ml is the estimate under the full model and is the one to hold against
    D_model.

    anomalous (default None: the code path without it): a dict with keys among exposure and sigma2 ({} for the defaults), the
    arguments of helpers/msd.estimate_anomalous_ml (csrc/fbm_ml.hip), the maximum-likelihood anomalous exponent of every
    track with a standard error.  exposure in [0, 1] is the part of a frame over which the camera integrates (default 0);
    sigma2 follows the rules of ml["sigma2"], and so do the rows used and the positions (drift-corrected, the frames of the
    table, a filled row is a gap).  The result gains alpha_ml, alpha_ml_std, D_alpha (float64) and anomalous_status (int64)
    [n_tracks], and "anomalous": what estimate_anomalous_ml was called with (positions, variances, frames, use, exposure).
    Tracks only: segments and states do not get an exponent of their own.

    confined (default None: the code path without it): a dict that may hold sigma2 ({} for the default), the argument of
    helpers/msd.estimate_confinement_ml (csrc/confined_ml.hip), the maximum-likelihood confinement radius of every track
    with a standard error and the likelihood ratio against free Brownian motion; the exposure is instantaneous (motion blur
    is not modelled).  sigma2 follows the rules of ml["sigma2"], and so do the rows used and the positions (drift-corrected,
    the frames of the table, a filled row is a gap).  The result gains radius_ml, radius_ml_std, D_conf, lambda_ml,
    lr_confined (float64; estimate_confinement_ml's radius, radius_std, D_conf, lambda and lr_brownian) and confined_status
    (int64) [n_tracks], and "confined": what estimate_confinement_ml was called with (positions, variances, frames, use).
    Tracks only.

    directed (default None: the code path without it): a dict with keys among blur and sigma2 ({} for the defaults), the
    arguments of helpers/msd.estimate_directed_ml (csrc/directed_ml.hip), the maximum-likelihood velocity of every track
    with a standard error and the likelihood ratio against free diffusion.  blur and sigma2 follow the rules of ml, and so
    do the rows used and the positions (the frames of the table, a filled row is a gap); it runs after drift, so the
    velocity that all tracks share is gone and what it reports is each track's own.  The result gains velocity_ml,
    velocity_ml_std [n_tracks, 2] ((y, x) in pixels per unit of dt), speed_ml, speed_ml_std, D_dir, D_dir_std, lr_directed,
    p_directed (float64; estimate_directed_ml's velocity, velocity_std, speed, speed_std, D_dir, D_dir_std, lr_brownian and
    p_brownian) and directed_status (int64) [n_tracks], and "directed": what estimate_directed_ml was called with (positions,
    variances, frames, use, blur).  Tracks only: the function takes any CSR offsets, so segments["seg_offsets"] or
    states["run_offsets"] can be passed to it with the arguments reported here.

    transport (default None: the code path without it): a dict of helpers/msd.segment_transport arguments (min_len, penalty,
    velocity_penalty, min_var, classes, blur; {} for the defaults; dt is this function's): run-and-pause tracks, whose VELOCITY
    changes along the track.  The result gains "transport": the segment_transport dict computed on the positions segment
    uses (drift-corrected if drift is given; csrc/segment.hip), plus n_sequences and D_model [n_seg] from the windows of
    plan_sequences(seg_offsets, seq_len, tail) exactly as for segment, so that no window straddles a cut.  With directed given
    it also holds velocity_ml, velocity_ml_std [n_seg, 2], speed_ml, D_dir, D_dir_std, lr_directed, p_directed and
    directed_status per stretch (estimate_directed_ml on seg_offsets with the arguments reported under "directed"), and with
    ml given D_ml, D_ml_std and ml_status per stretch.  Per track the result gains run_fraction (float64 [n_tracks]: the share
    of a track's rows that lie in directed stretches) and n_runs (int64 [n_tracks]: its directed stretches).  Every other
    entry is unchanged."""
    if transport is not None and (not isinstance(transport, dict) or set(transport) - set(_TRANSPORT_KEYS)):
        raise ValueError(f"transport must be None or a dict with keys among {', '.join(_TRANSPORT_KEYS)}")
    if directed is not None:
        if not isinstance(directed, dict) or set(directed) - {"blur", "sigma2"}:
            raise ValueError("directed must be None or a dict with keys among blur and sigma2")
        directed = dict(directed)
        directed.setdefault("blur", 0.0)
        directed.setdefault("sigma2", "crlb" if localization is not None else 0.0)
        if isinstance(directed["sigma2"], str):
            if directed["sigma2"] != "crlb":
                raise ValueError(f"directed['sigma2'] must be a number or 'crlb', got {directed['sigma2']!r}")
            if localization is None:
                raise ValueError("directed['sigma2'] = 'crlb' needs localization: the least-squares fit returns no bound")
        elif not 0.0 <= float(directed["sigma2"]) < float("inf"):
            raise ValueError(f"directed['sigma2'] must be >= 0 and finite, got {directed['sigma2']}")
        if not 0.0 <= float(directed["blur"]) <= 0.25:
            raise ValueError(f"directed['blur'] must lie in [0, 1/4], got {directed['blur']}")
    if confined is not None:
        if not isinstance(confined, dict) or set(confined) - {"sigma2"}:
            raise ValueError("confined must be None or a dict that may hold sigma2")
        confined = dict(confined)
        confined.setdefault("sigma2", "crlb" if localization is not None else 0.0)
        if isinstance(confined["sigma2"], str):
            if confined["sigma2"] != "crlb":
                raise ValueError(f"confined['sigma2'] must be a number or 'crlb', got {confined['sigma2']!r}")
            if localization is None:
                raise ValueError("confined['sigma2'] = 'crlb' needs localization: the least-squares fit returns no bound")
        elif not 0.0 <= float(confined["sigma2"]) < float("inf"):
            raise ValueError(f"confined['sigma2'] must be >= 0 and finite, got {confined['sigma2']}")
    if anomalous is not None:
        if not isinstance(anomalous, dict) or set(anomalous) - {"exposure", "sigma2"}:
            raise ValueError("anomalous must be None or a dict with keys among exposure and sigma2")
        anomalous = dict(anomalous)
        anomalous.setdefault("exposure", 0.0)
        anomalous.setdefault("sigma2", "crlb" if localization is not None else 0.0)
        if isinstance(anomalous["sigma2"], str):
            if anomalous["sigma2"] != "crlb":
                raise ValueError(f"anomalous['sigma2'] must be a number or 'crlb', got {anomalous['sigma2']!r}")
            if localization is None:
                raise ValueError("anomalous['sigma2'] = 'crlb' needs localization: the least-squares fit returns no bound")
        elif not 0.0 <= float(anomalous["sigma2"]) < float("inf"):
            raise ValueError(f"anomalous['sigma2'] must be >= 0 and finite, got {anomalous['sigma2']}")
        if not 0.0 <= float(anomalous["exposure"]) <= 1.0:
            raise ValueError(f"anomalous['exposure'] must lie in [0, 1], got {anomalous['exposure']}")
    if ml is not None:
        if not isinstance(ml, dict) or set(ml) - {"blur", "sigma2"}:
            raise ValueError("ml must be None or a dict with keys among blur and sigma2")
        ml = dict(ml)
        ml.setdefault("blur", 0.0)
        ml.setdefault("sigma2", "crlb" if localization is not None else 0.0)
        if isinstance(ml["sigma2"], str):
            if ml["sigma2"] != "crlb":
                raise ValueError(f"ml['sigma2'] must be a number or 'crlb', got {ml['sigma2']!r}")
            if localization is None:
                raise ValueError("ml['sigma2'] = 'crlb' needs localization: the least-squares fit returns no bound")
        elif not 0.0 <= float(ml["sigma2"]) < float("inf"):
            raise ValueError(f"ml['sigma2'] must be >= 0 and finite, got {ml['sigma2']}")
        if not 0.0 <= float(ml["blur"]) <= 0.25:
            raise ValueError(f"ml['blur'] must lie in [0, 1/4], got {ml['blur']}")
    neighbours = None
    if localization is not None:
        if not isinstance(localization, dict) or set(localization) - set(_CAMERA_KEYS) - {"neighbours"}:
            raise ValueError(f"localization must be None or a dict with keys among {', '.join(_CAMERA_KEYS)} and neighbours")
        neighbours = localization.get("neighbours")
        localization = {k: v for k, v in localization.items() if k != "neighbours"}
        if _check_neighbours(neighbours, "mle", (), patch_size) is None:
            neighbours = None
        if not refine:
            raise ValueError("localization needs refine=True: it is the refinement")
    if tracking_kwargs.get("detector") is not None:
        # the detector looks through the camera of the fit: gain, offset, read_var and sigma0 it does not name are localization's
        det = _check_detector(tracking_kwargs["detector"], localization)
        tracking_kwargs["detector"] = {"method": "lrt", **det}
    if isinstance(states, dict) and isinstance(states.get("sigma2"), str):
        if states["sigma2"] != "crlb":
            raise ValueError(f"states['sigma2'] must be a number or 'crlb', got {states['sigma2']!r}")
        if localization is None:
            raise ValueError("states['sigma2'] = 'crlb' needs localization: the least-squares fit returns no bound")
    if drift is not None and (not isinstance(drift, dict) or set(drift) - {"estimator", "smoothing", "min_pairs"}):
        raise ValueError("drift must be None or a dict with keys among estimator, smoothing and min_pairs")
    if states is not None:
        if not isinstance(states, dict) or set(states) - {"K", "sigma2", "max_iter", "tol", "min_var", "init"}:
            raise ValueError("states must be None or a dict with keys among K, sigma2, max_iter, tol, min_var and init")
        if "K" not in states:
            raise ValueError("states needs the number of states K")
    if not _is_cuda(movie):
        raise ValueError("estimate_track_diffusion needs a CUDA movie; move it to the GPU (movie.cuda())")
    if segment is not None and (not isinstance(segment, dict) or set(segment) - {"min_len", "penalty", "min_var", "blur"}):
        raise ValueError("segment must be None or a dict with keys among min_len, penalty, min_var and blur")
    _check_sequence_args(seq_len, tail, patch_size)
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size}")
    from .. import ops
    tracking_kwargs.setdefault("return_dog", False)
    table, _ = track_particles_tensors(movie, **tracking_kwargs)
    by_track = tracks_table_by_track(table)
    fr, y, x, tid, offsets = by_track[:5]
    lengths = offsets[1:] - offsets[:-1]
    n_tracks = len(lengths)
    movie = movie.float()
    located, from_crlb = None, False
    if refine and localization is not None:
        fit = refine_localizations_tensors(extract_patches_flat(movie, fr, y, x, patch_size), y, x, method="mle",
                                           camera=localization, **({"frames": fr, "neighbours": neighbours} if neighbours is not None else {}))
        pos = torch.stack([fit["y_refined"], fit["x_refined"]], dim=1)
        located = {k: fit[k] for k in ("y_std", "x_std", "photons", "background", "psf_size", "deviance", "status")
                   + (("n_neighbours", "neighbour", "photons_neighbour") if neighbours is not None else ())}
        var_row = (fit["y_std"] * fit["y_std"] + fit["x_std"] * fit["x_std"]) / 2.0
        good = fit["status"] == 0
        if len(by_track) > 5:
            good = good & ~by_track[5]
        row_of = torch.repeat_interleave(torch.arange(n_tracks, device=movie.device), lengths)
        zero = torch.zeros((), dtype=torch.float64, device=movie.device)
        n_good = torch.bincount(row_of[good], minlength=n_tracks)
        sigma2_loc = torch.zeros(n_tracks, dtype=torch.float64, device=movie.device).index_add_(
            0, row_of, torch.where(good, var_row, zero)) / n_good
        sigma2_loc = torch.where(n_good > 0, sigma2_loc, torch.full_like(sigma2_loc, float("nan")))
        if states is not None and states.get("sigma2") == "crlb":
            if not bool(good.any()):
                raise ValueError("states['sigma2'] = 'crlb': no row of the movie has a converged fit")
            states, from_crlb = dict(states, sigma2=float(var_row[good].mean())), True
    elif refine:
        fit = refine_localizations_tensors(extract_patches_flat(movie, fr, y, x, patch_size), y, x)
        pos = torch.stack([fit["y_refined"], fit["x_refined"]], dim=1)
    else:
        pos = torch.stack([y, x], dim=1).double()
    drifted = None
    if drift is not None:
        from . import msd as _msd
        drifted = _msd.estimate_drift(pos, fr, offsets, n_frames=movie.shape[0],
                                      use=~by_track[5] if len(by_track) > 5 else None, **drift)
        pos = _msd.subtract_drift(pos, fr, drifted["drift"])
        drifted["positions"] = pos
    msd, d_lstsq, d_weighted = ops.track_msd(pos, offsets.int(), float(dt), 0)
    if ml is not None:
        from . import msd as _msd
        filled = by_track[5] if len(by_track) > 5 else None
        if ml["sigma2"] == "crlb":
            ml_args = {"variances": torch.stack([fit["y_std"] * fit["y_std"], fit["x_std"] * fit["x_std"]], dim=1), "use": good}
        else:
            ml_args = {"variances": float(ml["sigma2"]), "use": None if filled is None else ~filled}
        ml_args.update(frames=fr, blur=float(ml["blur"]))

        def ml_fit(csr):
            return _msd.estimate_diffusion_ml(pos, csr, dt=dt, **ml_args)

        ml_tracks = ml_fit(offsets)
    if anomalous is not None:
        from . import msd as _msd
        filled = by_track[5] if len(by_track) > 5 else None
        if anomalous["sigma2"] == "crlb":
            an_args = {"variances": torch.stack([fit["y_std"] * fit["y_std"], fit["x_std"] * fit["x_std"]], dim=1), "use": good}
        else:
            an_args = {"variances": float(anomalous["sigma2"]), "use": None if filled is None else ~filled}
        an_args.update(frames=fr, exposure=float(anomalous["exposure"]))
        an_tracks = _msd.estimate_anomalous_ml(pos, offsets, dt=dt, **an_args)
    if confined is not None:
        from . import msd as _msd
        filled = by_track[5] if len(by_track) > 5 else None
        if confined["sigma2"] == "crlb":
            cf_args = {"variances": torch.stack([fit["y_std"] * fit["y_std"], fit["x_std"] * fit["x_std"]], dim=1), "use": good}
        else:
            cf_args = {"variances": float(confined["sigma2"]), "use": None if filled is None else ~filled}
        cf_args.update(frames=fr)
        cf_tracks = _msd.estimate_confinement_ml(pos, offsets, dt=dt, **cf_args)
    if directed is not None:
        from . import msd as _msd
        filled = by_track[5] if len(by_track) > 5 else None
        if directed["sigma2"] == "crlb":
            dm_args = {"variances": torch.stack([fit["y_std"] * fit["y_std"], fit["x_std"] * fit["x_std"]], dim=1), "use": good}
        else:
            dm_args = {"variances": float(directed["sigma2"]), "use": None if filled is None else ~filled}
        dm_args.update(frames=fr, blur=float(directed["blur"]))
        dm_tracks = _msd.estimate_directed_ml(pos, offsets, dt=dt, **dm_args)
    seq, seq_track, _ = track_sequences(movie, fr, y, x, offsets, seq_len, patch_size, norm, tail)
    n_sequences = torch.bincount(seq_track, minlength=n_tracks)
    model.eval()

    def mean_per_group(seq, counts):
        outs = []
        with torch.no_grad():
            for b0 in range(0, len(seq), int(batch_size)):
                out = model(seq[b0:b0 + int(batch_size)])
                outs.append(out.reshape(len(out), -1)[:, 0].double())
        per_seq = torch.cat(outs) if outs else torch.zeros(0, dtype=torch.float64, device=movie.device)
        d_model = torch.full((len(counts),), float("nan"), dtype=torch.float64, device=movie.device)
        if len(per_seq):
            d_model = torch.where(counts > 0, torch.segment_reduce(per_seq, "mean", lengths=counts), d_model)
        return d_model

    d_model = mean_per_group(seq, n_sequences)
    segments = None
    if segment is not None:
        from . import msd as _msd
        segments = _msd.segment_tracks(pos, offsets, dt=dt, **segment)
        seg_seq, seg_of_seq, _ = track_sequences(movie, fr, y, x, segments["seg_offsets"], seq_len, patch_size, norm, tail)
        segments["n_sequences"] = torch.bincount(seg_of_seq, minlength=len(segments["seg_track"]))
        segments["D_model"] = mean_per_group(seg_seq, segments["n_sequences"])
        if ml is not None:
            got = ml_fit(segments["seg_offsets"])
            segments["D_ml"], segments["D_ml_std"], segments["ml_status"] = got["D_ml"], got["D_ml_std"], got["status"]
    transported = None
    if transport is not None:
        from . import msd as _msd
        transported = _msd.segment_transport(pos, offsets, dt=dt, **transport)
        tr_seq, tr_of_seq, _ = track_sequences(movie, fr, y, x, transported["seg_offsets"], seq_len, patch_size, norm, tail)
        transported["n_sequences"] = torch.bincount(tr_of_seq, minlength=len(transported["seg_track"]))
        transported["D_model"] = mean_per_group(tr_seq, transported["n_sequences"])
        if directed is not None:
            got = _msd.estimate_directed_ml(pos, transported["seg_offsets"], dt=dt, **dm_args)
            for k, key in (("velocity_ml", "velocity"), ("velocity_ml_std", "velocity_std"), ("speed_ml", "speed"), ("D_dir", "D_dir"),
                           ("D_dir_std", "D_dir_std"), ("lr_directed", "lr_brownian"), ("p_directed", "p_brownian"),
                           ("directed_status", "status")):
                transported[k] = got[key]
        if ml is not None:
            got = ml_fit(transported["seg_offsets"])
            transported["D_ml"], transported["D_ml_std"], transported["ml_status"] = got["D_ml"], got["D_ml_std"], got["status"]
    fitted = None
    if states is not None:
        from . import msd as _msd
        fitted = _msd.fit_diffusion_states(pos, offsets, dt=dt, **states)
        if from_crlb:
            fitted["sigma2"] = float(states["sigma2"])
        st = fitted["state"]
        first = torch.zeros(len(st), dtype=torch.bool, device=movie.device)
        first[1:] = st[1:] != st[:-1]
        first[offsets[:-1][lengths > 0]] = True                            # a track's first row always starts a run
        first = torch.nonzero(first, as_tuple=True)[0]
        fitted["run_offsets"] = torch.cat([first, torch.full((1,), len(st), dtype=torch.int64, device=movie.device)])
        fitted["run_track"] = torch.searchsorted(offsets.long().contiguous(), first, right=True) - 1
        fitted["run_state"] = st[first]
        run_seq, run_of_seq, _ = track_sequences(movie, fr, y, x, fitted["run_offsets"], seq_len, patch_size, norm, tail)
        fitted["n_sequences"] = torch.bincount(run_of_seq, minlength=len(first))
        fitted["D_model"] = mean_per_group(run_seq, fitted["n_sequences"])
        if ml is not None:
            got = ml_fit(fitted["run_offsets"])
            fitted["D_ml"], fitted["D_ml_std"], fitted["ml_status"] = got["D_ml"], got["D_ml_std"], got["status"]
    res = {"track_id": tid[offsets[:-1]], "length": lengths, "n_sequences": n_sequences, "D_model": d_model,
           "D_msd": d_lstsq, "D_msd_weighted": d_weighted, "msd": msd}
    if len(by_track) > 5:
        row_track = torch.repeat_interleave(torch.arange(n_tracks, device=movie.device), lengths)
        res["n_filled"] = torch.bincount(row_track[by_track[5]], minlength=n_tracks)
    if segments is not None:
        res["segments"] = segments
    if fitted is not None:
        res["states"] = fitted
    if transported is not None:
        res["transport"] = transported
        res["run_fraction"], res["n_runs"] = transport_per_track(transported["seg_offsets"], transported["seg_track"],
                                                                 transported["seg_class"], lengths)
    if drifted is not None:
        res["drift"] = drifted
    if located is not None:
        res["localization"], res["sigma2_loc"] = located, sigma2_loc
    if ml is not None:
        res["D_ml"], res["D_ml_std"], res["ml_status"] = ml_tracks["D_ml"], ml_tracks["D_ml_std"], ml_tracks["status"]
        res["ml"] = dict(ml_args, positions=pos)
    if anomalous is not None:
        res["alpha_ml"], res["alpha_ml_std"], res["D_alpha"] = an_tracks["alpha_ml"], an_tracks["alpha_ml_std"], an_tracks["D_alpha"]
        res["anomalous_status"] = an_tracks["status"]
        res["anomalous"] = dict(an_args, positions=pos)
    if confined is not None:
        res["radius_ml"], res["radius_ml_std"], res["D_conf"] = cf_tracks["radius"], cf_tracks["radius_std"], cf_tracks["D_conf"]
        res["lambda_ml"], res["lr_confined"], res["confined_status"] = cf_tracks["lambda"], cf_tracks["lr_brownian"], cf_tracks["status"]
        res["confined"] = dict(cf_args, positions=pos)
    if directed is not None:
        for k, key in (("velocity_ml", "velocity"), ("velocity_ml_std", "velocity_std"), ("speed_ml", "speed"),
                       ("speed_ml_std", "speed_std"), ("D_dir", "D_dir"), ("D_dir_std", "D_dir_std"), ("lr_directed", "lr_brownian"),
                       ("p_directed", "p_brownian"), ("directed_status", "status")):
            res[k] = dm_tracks[key]
        res["directed"] = dict(dm_args, positions=pos)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# scoring against a simulated field of view (helpers/generation.simulate_movie)
# ----------------------------------------------------------------------------------------------------------------------
def score_tracking(frame, y, x, track_id, truth, max_distance=2.0):
    """How well a detections table (frame, y, x, track_id [N]; arrays or tensors, integer or refined positions) recovers the
    truth table of generation.simulate_movie.  Torch ops on the inputs' device, no loop over frames or tracks.

    Every detection is matched to the nearest truth particle visible in its frame (ties: the lowest particle_id), if that is
    within max_distance pixels.  -> dict of tensors on that device:
      recall      distinct truth rows that some detection matched / truth rows           (0-dim float64; NaN without truth rows)
      precision   distinct truth rows matched / detections: a second detection on the same particle-frame counts against it
      rmse        root mean square distance over the matched detections                   (NaN without a match)
      n_detections, n_truth, n_matched (0-dim int64; n_matched counts detections)
      matched_particle [N] int64, the particle each detection was matched to or -1
      track_id [n_tracks] the distinct ids ascending, and per track: n_rows, particle_id (the particle most of its rows were
      matched to; ties: the lowest; -1 if none was matched), purity (rows matched to that particle / all rows of the track)
      and D_true (truth["D"] of that particle, NaN for -1)."""
    dev = None
    for v in (frame, y, x, track_id):
        if torch.is_tensor(v):
            dev = v.device
            break
    fr = torch.as_tensor(frame, device=dev).long()
    dev = fr.device
    yy, xx = torch.as_tensor(y, device=dev).double(), torch.as_tensor(x, device=dev).double()
    tid = torch.as_tensor(track_id, device=dev).long()
    if not (fr.dim() == 1 and fr.shape == yy.shape == xx.shape == tid.shape):
        raise ValueError("frame, y, x and track_id must be 1-D with one entry per detection")
    md = float(max_distance)
    if not md >= 0:
        raise ValueError(f"max_distance must be >= 0, got {max_distance}")
    t_fr, t_pid = truth["frame"].to(dev).long(), truth["particle_id"].to(dev).long()
    t_y, t_x, t_D = truth["y"].to(dev).double(), truth["x"].to(dev).double(), truth["D"].to(dev).double()
    Np, n_truth, n_det = t_D.numel(), t_fr.numel(), fr.numel()
    n_frames = int(torch.cat([t_fr, fr]).max()) + 1 if n_truth + n_det else 1
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    if Np and n_det:
        ty = torch.full((n_frames, Np), float("inf"), dtype=torch.float64, device=dev)      # inf: not visible in that frame
        tx = torch.full((n_frames, Np), float("inf"), dtype=torch.float64, device=dev)
        ty[t_fr, t_pid], tx[t_fr, t_pid] = t_y, t_x
        inside = fr >= 0
        f_ = fr.clamp_min(0)
        d2 = (ty[f_] - yy[:, None]) ** 2 + (tx[f_] - xx[:, None]) ** 2                      # [N, Np]
        dmin2, who = d2.min(dim=1)                                                          # first minimum: lowest particle_id
        ok = inside & (dmin2 <= md * md)
    else:
        dmin2 = torch.zeros(n_det, dtype=torch.float64, device=dev)
        who = torch.zeros(n_det, dtype=torch.int64, device=dev)
        ok = torch.zeros(n_det, dtype=torch.bool, device=dev)
    matched = torch.where(ok, who, torch.full_like(who, -1))
    n_matched = ok.sum()
    distinct = torch.unique(fr[ok] * max(Np, 1) + who[ok]).numel()
    distinct = torch.full((), float(distinct), dtype=torch.float64, device=dev)
    tracks, tidx = torch.unique(tid, return_inverse=True)
    n_tracks = tracks.numel()
    n_rows = torch.bincount(tidx, minlength=n_tracks)
    votes = torch.bincount(tidx[ok] * max(Np, 1) + who[ok], minlength=n_tracks * max(Np, 1)).view(n_tracks, max(Np, 1))
    top, major = votes.max(dim=1) if n_tracks else (n_rows, n_rows)
    major = torch.where(top > 0, major, torch.full_like(major, -1))
    d_true = torch.where(major >= 0, t_D[major.clamp_min(0)], nan) if Np else torch.full((n_tracks,), float("nan"),
                                                                                       dtype=torch.float64, device=dev)
    return {"recall": distinct / n_truth if n_truth else nan, "precision": distinct / n_det if n_det else nan,
            "rmse": torch.sqrt(dmin2[ok].sum() / n_matched) if n_det else nan,
            "n_detections": torch.full((), n_det, dtype=torch.int64, device=dev),
            "n_truth": torch.full((), n_truth, dtype=torch.int64, device=dev), "n_matched": n_matched,
            "matched_particle": matched, "track_id": tracks, "n_rows": n_rows, "particle_id": major,
            "purity": top.double() / n_rows.double().clamp_min(1.0), "D_true": d_true}
