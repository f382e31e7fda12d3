"""fp64 reference, domain predicate, fp32 yardstick, error model, launcher restatement and case table of
tests/test_render_frames.py (CPU) and tests/test_render_frames_gpu.py (csrc/render.hip, mivit_render_frames, and its caller
helpers/generation.render_frames).  Plain numpy.

The operation (reference helpers/helpersGeneration.py:283-319): per frame, npos Gaussian spots of width sigma on the grid
linspace(-limit, limit, G), G = P * up, limit = (G - 1) // 2, each divided by its own maximum ON THAT GRID and multiplied by
its amplitude, summed, then mean-pooled up x up.

Error model.  A stored pixel is v = sum_p a_p py_p[y] px_p[x], every profile value a mean of `up` exponentials
exp(arg), arg = -((g - c)^2 - (g* - c)^2) / 2 sigma^2 (g a fine-grid point, g* the grid point nearest to the spot's
position c).  In fp32 an exponential carries the relative error of the exponential itself plus the ABSOLUTE error of its
argument, which is a few fp32 roundings of |arg|.  So the error of sub-position p's term is its magnitude times
c_exp + c_arg * A_p, A_p = |arg| of the pixel (row part + column part), and the pixel's is

    E[y, x] = sum_p |a_p| py_p[y] px_p[x] (c_exp + c_arg (Ay_p[y] + Ax_p[x]))  =  c_exp B + c_arg W.

A pixel's |arg| is that of its `up` fine samples weighted by what each contributes, Ax_p px_p = mean_k exp(arg_k) |arg_k|,
not their maximum: on the border pixel next to a narrow spot outside the frame one sample is the peak itself (arg = 0,
weight 1) and its neighbour has |arg| = 20 and weight e^-20; the maximum would grant that pixel 20 roundings it cannot use
(with it, an exponential of the peak sample that was 1.5e-5 away from 1 passed).

with magnitudes and arguments from the fp64 profiles, plus the underflow floor UF = 2^-126 (1 + sum_p |a_p|): below the
smallest normal fp32 number an exponential, a profile or a product has an absolute error, not a relative one (a GPU
exponential may flush there), each at most 2^-126 and each multiplied by at most |a_p|.  The reference has a floor of its
own, RU = sum_p |a_p| 2^-1074 / spot_p.max(): it divides the G x G spot by its maximum, and where the spot is below the
smallest fp64 subnormal it is 0 (with a peak of 1e-300, in the far entries, that is 1e-24 of the peak; nothing in fp32
terms, but more than nothing).  UF + RU is written U below.  Neither constant is chosen: both are measured on the
yardstick, an fp32 restatement of the formula in numpy (np.exp, the argument in the factored form (d - dpk) (d + dpk), the kernel's
order of operations) run on the same inputs and compared with the fp64 reference:
    c_exp = the worst |yardstick - ref| / B over the pixels of the WHOLE table whose weighted argument W / B is <= 1 (an
            argument that small has an absolute rounding error below 2^-24: what is left is the exponential, the mean
            and the sum), never below one fp32 rounding.  One value for the entries whose grid is exact in fp32 (odd G:
            step == 1; G <= 2: step == 0) and one for the others (even G: the points -limit + i * step, step = 2 limit /
            (G - 1), are rounded, and that error times the slope of the argument does not vanish with the argument);
    c_arg = per case, the smallest constant with |yardstick - ref| <= c_exp B + c_arg W + U on every pixel of the case, never
            below one fp32 rounding (the argument is an fp32 number).  It is per case because it is the conditioning of
            the case: with an even G the grid points -limit + i * step are themselves rounded, with center=True the
            centre is an fp32 mean, and both errors are multiplied by the slope of the argument.
The code under test gets 4 E (the margin operators_common.measured_bar gives a transcendental kernel over its fp32
restatement) plus FLOOR_ROUNDINGS fp32 roundings of the pixel's magnitude B.  The old bound 2e-5 * max|ref| of
tests/test_generation_gpu.py stays as an outer check, per case.
"""
import functools

import numpy as np

U32 = 2.0 ** -24
OUTER = 2e-5                 # the bound of tests/test_generation_gpu.py, relative to the case's largest |ref|
MARGIN = 4.0                 # operators_common.measured_bar
FLOOR_ROUNDINGS = 4.0
LDS_CAP = 64 * 1024          # csrc/render.hip: the launcher's bound
MAX_GRID = 65535             # grid.y / grid.z: sequences and PSF widths per launch
THREADS = 256
TINY64 = float(np.finfo(np.float64).tiny)
TINY32 = 2.0 ** -126
DENORM64 = 2.0 ** -1074


# ---------------------------------------------------------------------------------------------------------------------
# launcher restatement (csrc/render.hip)
# ---------------------------------------------------------------------------------------------------------------------
def lds_bytes(npos, P):
    return (2 * npos * P + npos + 2) * 4


def lds_max_npos(P):
    """the largest npos the launcher accepts at frame side P"""
    n = 1
    while lds_bytes(n + 1, P) <= LDS_CAP:
        n += 1
    return n


def grid32(P, up):
    """-> G, limit, step as the kernel computes them (fp32)"""
    G = P * up
    limit = (G - 1) // 2
    step = np.float32(2) * np.float32(limit) / np.float32(G - 1) if G > 1 else np.float32(0)
    return G, limit, np.float32(step)


def centred32(traj, npos, center):
    """fp32 [N, F, npos, 2]: sub-positions minus the frame's centre, the centre summed in sequence and divided as the kernel does"""
    N, T, _ = traj.shape
    seg = np.asarray(traj, np.float32).reshape(N, T // npos, npos, 2)
    cen = np.zeros((N, T // npos, 1, 2), np.float32)
    if center:
        for p in range(npos):
            cen[:, :, 0] += seg[:, :, p]
        cen = cen / np.float32(npos)
    return seg - cen


def peak_index32(c, P, up):
    """the kernel's gi BEFORE the clamp, and after: rint((c + limit) / step)"""
    G, limit, step = grid32(P, up)
    raw = np.rint((c + np.float32(limit)) / step) if step > 0 else np.zeros_like(c)
    return raw, np.clip(raw, np.float32(0), np.float32(G - 1))


# ---------------------------------------------------------------------------------------------------------------------
# fp64 reference: the definition
# ---------------------------------------------------------------------------------------------------------------------
def reference(traj, npos, sigmas, P, up, amp, center, chunk=16):
    """-> (frames [N, nsig, F, P, P] fp64, peaks [N, nsig, F, npos]: every spot's own maximum on the fine grid).
    The loops of tests/test_generation_gpu.naive_frames with the G x G spots of `chunk` sub-positions evaluated at once."""
    traj = np.asarray(traj, np.float64)
    N, T, _ = traj.shape
    F, G = T // npos, P * up
    amp = np.broadcast_to(np.asarray(amp, np.float64), (N, F, npos))
    limit = (G - 1) // 2
    axis = np.linspace(-limit, limit, G)
    out = np.zeros((N, len(sigmas), F, P, P))
    peaks = np.zeros((N, len(sigmas), F, npos))
    with np.errstate(all="ignore"):
        for n in range(N):
            for f in range(F):
                seg = traj[n, f * npos:(f + 1) * npos]
                if center:
                    seg = seg - seg.mean(axis=0)
                for si, s in enumerate(sigmas):
                    hr = np.zeros((G, G))
                    for p0 in range(0, npos, chunk):
                        x = seg[p0:p0 + chunk, 0, None, None] * up
                        y = seg[p0:p0 + chunk, 1, None, None] * up
                        spot = np.exp(-((axis[None, None, :] - x) ** 2 + (axis[None, :, None] - y) ** 2) / (2 * s * s))
                        mx = spot.max(axis=(1, 2))
                        peaks[n, si, f, p0:p0 + chunk] = mx
                        for q in range(spot.shape[0]):
                            hr += amp[n, f, p0 + q] / mx[q] * spot[q]
                    out[n, si, f] = hr.reshape(P, up, P, up).mean(axis=(1, 3))
    return out, peaks


def ref_floor(amp, peaks):
    """RU [N, nsig, F, 1, 1]: what the reference itself may be off by, see the module docstring"""
    N, nsig, F, npos = peaks.shape
    a = np.abs(np.broadcast_to(np.asarray(amp, np.float64), (N, F, npos)))
    with np.errstate(all="ignore"):
        return (a[:, None] * DENORM64 / peaks).sum(axis=-1)[..., None, None]


def in_domain(peaks):
    """the reference divides by spot.max(): it means something only while that is a normal fp64 number"""
    return bool(np.isfinite(peaks).all() and (peaks >= TINY64).all())


# ---------------------------------------------------------------------------------------------------------------------
# fp64 profiles: magnitudes and arguments of the error model
# ---------------------------------------------------------------------------------------------------------------------
def profiles64(traj, npos, sigmas, P, up, center):
    """-> prof, profA [N, nsig, F, npos, 2 (x, y), P]: pooled peak-normalised 1-D profiles mean_k exp(arg_k), and
    mean_k exp(arg_k) |arg_k|"""
    traj = np.asarray(traj, np.float64)
    N, T, _ = traj.shape
    F, G = T // npos, P * up
    limit = (G - 1) // 2
    axis = np.linspace(-limit, limit, G)
    seg = traj.reshape(N, F, npos, 2)
    if center:
        seg = seg - seg.mean(axis=2, keepdims=True)
    d = axis - (seg * up)[..., None]                                        # [N, F, npos, 2, G]
    dpk = np.take_along_axis(d, np.abs(d).argmin(axis=-1)[..., None], axis=-1)
    prof, A = [], []
    for s in sigmas:
        arg = -((d - dpk) * (d + dpk)) / (2 * s * s)
        prof.append(np.exp(arg).reshape(N, F, npos, 2, P, up).mean(axis=-1))
        A.append((np.exp(arg) * np.abs(arg)).reshape(N, F, npos, 2, P, up).mean(axis=-1))
    return np.stack(prof, axis=1), np.stack(A, axis=1)


def magnitudes(traj, npos, sigmas, P, up, amp, center):
    """-> B, W, S, UF [N, nsig, F, P, P]: sum_p |a_p| py px, the same weighted by (Ay + Ax), the signed sum (the separable
    form of the reference: the CPU half checks it against the 2-D definition), and the fp32 underflow floor"""
    N, T, _ = np.shape(traj)
    a = np.broadcast_to(np.asarray(amp, np.float64), (N, T // npos, npos))
    prof, A = profiles64(traj, npos, sigmas, P, up, center)
    px, py, pxA, pyA = prof[..., 0, :], prof[..., 1, :], A[..., 0, :], A[..., 1, :]
    es = "nfp,nsfpy,nsfpx->nsfyx"
    B = np.einsum(es, np.abs(a), py, px)
    W = np.einsum(es, np.abs(a), pyA, px) + np.einsum(es, np.abs(a), py, pxA)
    UF = np.broadcast_to(TINY32 * (1 + np.abs(a).sum(axis=-1))[:, None, :, None, None], B.shape)
    return B, W, np.einsum(es, a, py, px), UF


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick: the same formula in fp32, factored argument, the kernel's order of operations
# ---------------------------------------------------------------------------------------------------------------------
def yardstick32(traj, npos, sigmas, P, up, amp, center):
    f32 = np.float32
    N, T, _ = np.shape(traj)
    F = T // npos
    G, limit, step = grid32(P, up)
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(amp, f32), (N, F, npos)))
    c = centred32(traj, npos, center) * f32(up)                              # [N, F, npos, 2]
    _, gi = peak_index32(c, P, up)
    dpk = ((-f32(limit) + gi * step) - c)[..., None]
    g = -f32(limit) + np.arange(G, dtype=f32) * step
    d = g - c[..., None]                                                     # [N, F, npos, 2, G]
    out = np.zeros((N, len(sigmas), F, P, P), f32)
    for si, s in enumerate(sigmas):
        inv2s2 = f32(1) / (f32(2) * f32(s) * f32(s))
        e = np.exp(-((d - dpk) * (d + dpk)) * inv2s2).reshape(N, F, npos, 2, P, up)
        assert e.dtype == f32
        acc = np.zeros(e.shape[:-1], f32)
        for k in range(up):
            acc += e[..., k]
        prof = acc / f32(up)
        for p in range(npos):
            out[:, si] += (a[:, :, p, None, None] * prof[:, :, p, 1, :, None]) * prof[:, :, p, 0, None, :]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
PUP = [(1, 1), (1, 5), (2, 1), (2, 3), (8, 4), (9, 5), (13, 5), (9, 1), (7, 2), (16, 3), (32, 5), (64, 5)]
NARROW, WIDE = 0.3, 3.0                     # sigma on the fine grid, in units of up: narrower than a camera pixel .. 3 pixels
FAR = (0.5, 1.5, 4.0, 12.0)                 # distance outside the frame, in units of P
FAR_BUDGET = 690.0                          # -log(spot.max()) the far entries aim at most for; the fp64 normals end at 708.4


def sig32(*s):
    """sigmas as the fp32 values the kernel reads, so that every side computes with the same number"""
    return [float(np.float32(v)) for v in s]


def _amps(rng, N, F, npos):
    return (500 + 50 * rng.standard_normal((N, F, npos))).astype(np.float32)


def _traj(rng, N, F, npos, P, jitter=0.4):
    """frame centres uniform in the middle half of the frame, sub-positions scattered around them"""
    cen = rng.uniform(-P / 4, P / 4, (N, F, 1, 2))
    return (cen + jitter * rng.standard_normal((N, F, npos, 2))).reshape(N, F * npos, 2).astype(np.float32)


def far_distance(P, up, sigma, nominal, axes, jitter=0.5):
    """camera pixels beyond the frame's edge: `nominal`, shrunk until -log(spot.max()) = axes * e^2 / 2 sigma^2 <=
    FAR_BUDGET for the distance e (fine-grid steps) to the last grid point on each of `axes` axes, `jitter` pixels included"""
    e_max = np.sqrt(FAR_BUDGET * 2 * sigma * sigma / axes)
    return float(min(nominal, e_max / up - jitter))


def _case(cid, group, P, up, npos, sigmas, center, traj, amp, **reach):
    traj, amp = np.ascontiguousarray(traj, np.float32), np.ascontiguousarray(amp, np.float32)
    N, T, _ = traj.shape
    assert T % npos == 0 and amp.shape == (N, T // npos, npos)
    return dict(id=cid, group=group, P=P, up=up, npos=npos, sigmas=sig32(*sigmas), center=center, traj=traj, amp=amp, reach=reach)


def _far_cases():
    out = []
    sides = {"A": [(1, 0), (0, -1), (1, 1)], "B": [(-1, 0), (0, 1), (-1, 1)]}      # (sign x, sign y) per frame
    for P, up in ((9, 5), (8, 4)):
        half = ((P * up - 1) // 2) / up                                           # the last grid point, in camera pixels
        for wname, w in (("narrow", NARROW), ("wide", WIDE)):
            s = float(np.float32(w * up))
            for sname, sgn in sides.items():
                rng = np.random.default_rng(P * 1000 + up * 100 + (wname == "wide") * 10 + (sname == "B"))
                traj = np.zeros((len(FAR), len(sgn), 2, 2))
                for n, far in enumerate(FAR):
                    for f, (sx, sy) in enumerate(sgn):
                        dist = far_distance(P, up, s, far * P, abs(sx) + abs(sy))
                        base = np.array([sx * (half + dist), sy * (half + dist)])
                        inside = rng.uniform(-P / 4, P / 4, 2) * (np.array([sx, sy]) == 0)
                        # jitter towards the frame only, so that the budget holds
                        traj[n, f] = base + inside - np.array([sx, sy]) * rng.uniform(0, 0.5, (2, 2))
                out.append(_case(f"far-{P}x{up}-{wname}-{sname}", f"far-{wname}", P, up, 2, [s], False,
                                 traj.reshape(len(FAR), -1, 2), _amps(rng, len(FAR), len(sgn), 2), far=True, sides=sgn))
    return out


def _tie_cases():
    """center=False and positions that are exact in fp32 after the multiplication by up"""
    out = []
    # odd G, step == 1: the grid points are the integers, c = up * position
    for P in (9, 13):
        on = [(0.0, 0.0), (1.0, -2.0), (-3.0, 4.0), (float(P // 2), -float(P // 2))]          # c = 5 k: on a grid point
        half = [(0.5, 0.5), (-1.5, 2.5), (2.5, -0.5), (-3.5, 1.5)]                            # c = 5 k + 2.5: half-way
        traj = np.array([on, half], np.float64)                                               # [N = 2, T = 4, 2]
        out.append(_case(f"ties-{P}x5", "ties", P, 5, 2, [NARROW * 5, 2.3], False, traj, _amps(np.random.default_rng(P), 2, 2, 2),
                         on_grid=True, half_way=True))
    # even G: the two ends of the grid (+-limit) are grid points, and 0 lies half-way between the two middle ones
    for P, up in ((8, 4), (7, 2)):                             # limit / up is exact in fp32 for these
        lim = ((P * up - 1) // 2) / up
        on = [(lim, -lim), (-lim, lim)]
        half = [(0.0, 0.0), (0.0, lim)]
        traj = np.array([on, half], np.float64)
        out.append(_case(f"ties-{P}x{up}", "ties", P, up, 1, [NARROW * up, 1.1 * up], False, traj,
                         _amps(np.random.default_rng(P + up), 2, 2, 1), on_grid=True, half_way=True))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # every (P, up): G = 1, odd and even G, step == 0 (G = 2), P * P above 256 threads; center alternates
    for i, (P, up) in enumerate(PUP):
        rng = np.random.default_rng(100 + i)
        N, F = (1, 1) if P == 64 else (1, 2) if P == 32 else (2, 2)
        out.append(_case(f"grid-{P}x{up}", "grid", P, up, 2, [NARROW * up, WIDE * up], i % 2 == 0, _traj(rng, N, F, 2, P),
                         _amps(rng, N, F, 2)))
    for npos in (1, 2, 5, 10):
        for P, up, center in ((9, 5, True), (8, 4, False)):
            rng = np.random.default_rng(200 + npos * 10 + P)
            out.append(_case(f"npos{npos}-{P}x{up}", "npos", P, up, npos, [0.46 * up, 1.1 * up], center, _traj(rng, 2, 3, npos, P),
                             _amps(rng, 2, 3, npos)))
    for nsig in (1, 2, 5):
        for P, up, center in ((9, 5, False), (7, 2, True)):
            rng = np.random.default_rng(300 + nsig * 10 + P)
            sig = np.linspace(NARROW * up, WIDE * up, nsig) if nsig > 1 else [1.0 * up]
            out.append(_case(f"nsig{nsig}-{P}x{up}", "nsig", P, up, 3, sig, center, _traj(rng, 2, 2, 3, P), _amps(rng, 2, 2, 3)))
    for P, up, center in ((9, 5, True), (8, 4, False)):
        rng = np.random.default_rng(400 + P)
        amp = _amps(rng, 3, 2, 5)
        amp[0, 0, 1] = 0.0
        amp[0, 1, :] = 0.0                                  # a whole frame of exact zeros
        amp[1, 0, 2] = -300.0                               # a negative value among positive ones
        amp[2, 1, 4] = -0.0
        out.append(_case(f"amps-{P}x{up}", "amps", P, up, 5, [NARROW * up, 2.3], center, _traj(rng, 3, 2, 5, P), amp, zeros=True,
                         negative=True))
    out += _tie_cases()
    out += _far_cases()
    # one frame whose sub-positions walk from the middle of the frame to 1.7 P from it
    for P, up in ((9, 5), (8, 4)):
        rng = np.random.default_rng(500 + P)
        walk = np.linspace(0.0, 1.7 * P, 5)[None, :, None] * np.array([[[1.0, 0.0]], [[0.6, -0.8]]])      # [N = 2, 5, 2]
        traj = walk + 0.2 * rng.standard_normal((2, 5, 2))
        out.append(_case(f"straddle-{P}x{up}", "straddle", P, up, 5, [2.3, 1.5 * up], False, traj, _amps(rng, 2, 1, 5), straddle=True))
    # the largest npos the launcher's LDS check accepts at P = 64
    rng = np.random.default_rng(600)
    n_max = lds_max_npos(64)
    out.append(_case("lds-64x5", "lds", 64, 5, n_max, [2.0 * 5], True, _traj(rng, 1, 1, n_max, 64, jitter=3.0), _amps(rng, 1, 1, n_max),
                     lds_edge=True))
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)


def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def args(c):
    return c["traj"], c["npos"], c["sigmas"], c["P"], c["up"], c["amp"], c["center"]


# ---------------------------------------------------------------------------------------------------------------------
# the measured model
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table():
    """id -> dict(ref, peaks, B, W, S, yard, yerr); computed once and never changed (the arrays are read-only)"""
    out = {}
    for c in cases():
        ref, peaks = reference(*args(c))
        B, W, S, UF = magnitudes(*args(c))
        yard = yardstick32(*args(c)).astype(np.float64)
        rec = dict(ref=ref, peaks=peaks, B=B, W=W, S=S, UF=UF + ref_floor(c["amp"], peaks), yard=yard, yerr=np.abs(yard - ref))
        for v in rec.values():
            v.setflags(write=False)
        rec["id"] = c["id"]
        out[c["id"]] = rec
    return out


def exact_grid(P, up):
    G, _, step = grid32(P, up)
    return bool(step == 1 or step == 0)


@functools.lru_cache(maxsize=None)
def c_exp(exact):
    worst = U32
    for c in cases():
        if exact_grid(c["P"], c["up"]) != exact:
            continue
        rec = table()[c["id"]]
        m = (rec["B"] > 0) & (rec["W"] <= rec["B"]) & np.isfinite(rec["yerr"])
        if m.any():
            worst = max(worst, float(((rec["yerr"][m] - rec["UF"][m]) / rec["B"][m]).max()))
    return worst


def fit_c_arg(err, B, W, UF, ce):
    """the smallest c >= 2^-24 with err <= ce B + c W + UF wherever W > 0"""
    m = W > 0
    if not m.any():
        return U32
    return max(U32, float(((err[m] - ce * B[m] - UF[m]) / W[m]).max()))


@functools.lru_cache(maxsize=None)
def c_arg(cid):
    rec = table()[cid]
    return fit_c_arg(rec["yerr"], rec["B"], rec["W"], rec["UF"], case_c_exp(cid))


def case_c_exp(cid):
    c = case(cid)
    return c_exp(exact_grid(c["P"], c["up"]))


def yard_model(cid):
    rec = table()[cid]
    return case_c_exp(cid) * rec["B"] + c_arg(cid) * rec["W"] + rec["UF"]


def bar(cid):
    """per pixel: what the code under test may be off by"""
    return MARGIN * yard_model(cid) + FLOOR_ROUNDINGS * U32 * table()[cid]["B"]


def bar_for(traj, npos, sigmas, P, up, amp, center):
    """the same bar for inputs outside the table (wrapper and data-path tests): reference, and the constants measured on
    these very inputs' yardstick"""
    ref, peaks = reference(traj, npos, sigmas, P, up, amp, center)
    assert in_domain(peaks)
    B, W, _, UF = magnitudes(traj, npos, sigmas, P, up, amp, center)
    UF = UF + ref_floor(amp, peaks)
    err = np.abs(yardstick32(traj, npos, sigmas, P, up, amp, center).astype(np.float64) - ref)
    ce = c_exp(exact_grid(P, up))
    ca = fit_c_arg(err, B, W, UF, ce)
    return ref, MARGIN * (ce * B + ca * W + UF) + FLOOR_ROUNDINGS * U32 * B


def ratio(got, ref, b):
    """-> (worst |got - ref| / bar, that error, that bar, flat index); a pixel with bar 0 must be exact"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    r = np.where(err > 0, err / np.maximum(b, 1e-300), 0.0)
    i = int(r.argmax())
    return float(r.flat[i]), float(err.flat[i]), float(b.flat[i]), i


def outer_ok(got, ref):
    scale = float(np.abs(ref).max())
    worst = float(np.abs(np.asarray(got, np.float64) - ref).max())
    return worst < OUTER * scale or (scale == 0.0 and worst == 0.0), worst / max(scale, 1e-300)


def groups():
    return sorted({c["group"] for c in cases()})
