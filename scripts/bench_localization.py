"""Fits per second of the Poisson maximum-likelihood kernel (ops.fit_spots_mle -> csrc/localize.hip) with the width free and
with the width held, and of the least-squares kernel it stands beside (ops.refine_gaussian -> csrc/tracking.hip), on the same
GPU and the same Poisson patches: one emitter of 1000 photons, sigma 1.3, on 10 background photons per pixel, centres uniform
within half a pixel.  Events on the stream after a warm-up; every timed window repeats its call until it holds at least 0.2 s
of work, and the minimum of 5 windows is reported per call (the outputs are allocated inside the call, as a user's are).
N = 10^3, 10^5, 10^6 patches of side P = 7 and 9.  Also reported: the mean iterations per fit, the share of converged fits, and
whether two runs agree bit for bit.  Every GPU step is followed by a synchronisation and an error check of its own; the first
error ends the script with a non-zero status, nothing further is started.

--pairs times the joint two-emitter kernel instead (ops.fit_spots_mle2 -> csrc/localize2.hip): patches with a second emitter of
the same brightness 0.4 P away at a random angle, guesses at the nearest integers, width free, beside ops.fit_spots_mle on the
same patches for scale (that fit is the wrong model there; only its time is of interest), and the joint kernel with
count = 1 on the single-emitter patches.  N = 10^3, 10^4, 10^5.

    python scripts/bench_localization.py [--small-only] [--pairs] [--json OUT]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from moleculardiffusion_mivit_amd import ops

PHOTONS, BACKGROUND, SIGMA = 1000.0, 10.0, 1.3


def checked(what, fn):
    """one GPU step under its own check: run, wait for it, and leave on the first error"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as exc:                                 # noqa: BLE001  (whatever went wrong, nothing more is started)
        print(f"bench_localization: {what} failed: {exc}", file=sys.stderr, flush=True)
        sys.exit(1)


def t_events(fn, windows=5, min_window=0.2):
    fn()                                                     # warm-up: code object load, allocator
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(1, min(2000, int(min_window / max(a.elapsed_time(b) * 1e-3, 1e-6))))
    best = float("inf")
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3 / reps)
    return best


def poisson_patches(n, P, seed=0):
    """[n, P, P] float32 on the GPU, drawn there: Poisson counts of the pixel-integrated Gaussian on the background"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = P // 2 + torch.rand(2, n, 1, generator=g, device="cuda", dtype=torch.float64) - 0.5
    edges = torch.arange(P + 1, device="cuda", dtype=torch.float64) - 0.5
    e = torch.erf((edges[None, None, :] - c) / (math.sqrt(2.0) * SIGMA))
    E = 0.5 * (e[..., 1:] - e[..., :-1])
    mu = BACKGROUND + PHOTONS * E[1][:, :, None] * E[0][:, None, :]
    return torch.poisson(mu.float(), generator=g).contiguous()


def pair_patches(n, P, seed=0):
    """([n, P, P] float32, guess [n, 4] float64) on the GPU: poisson_patches with a second emitter 0.4 P away"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = P // 2 + torch.rand(2, n, 1, generator=g, device="cuda", dtype=torch.float64) - 0.5
    ang = 2.0 * math.pi * torch.rand(n, 1, generator=g, device="cuda", dtype=torch.float64)
    c2 = c + 0.4 * P * torch.stack([torch.cos(ang), torch.sin(ang)])
    edges = torch.arange(P + 1, device="cuda", dtype=torch.float64) - 0.5

    def spot(cc):
        e = torch.erf((edges[None, None, :] - cc) / (math.sqrt(2.0) * SIGMA))
        E = 0.5 * (e[..., 1:] - e[..., :-1])
        return PHOTONS * E[1][:, :, None] * E[0][:, None, :]

    mu = BACKGROUND + spot(c) + spot(c2)
    centre = torch.full((n,), float(P // 2), dtype=torch.float64, device="cuda")
    guess = torch.stack([centre, centre, torch.round(c2[0, :, 0]), torch.round(c2[1, :, 0])], dim=1).contiguous()
    return torch.poisson(mu.float(), generator=g).contiguous(), guess


def bench_pairs(n, P):
    patches, guess = checked("patches", lambda: pair_patches(n, P))
    alone = checked("patches", lambda: poisson_patches(n, P))
    two = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    one = torch.ones(n, dtype=torch.int32, device="cuda")
    out = {"N": n, "P": P}
    calls = (("mle2_pairs", lambda: ops.fit_spots_mle2(patches, two, guess, sigma0=SIGMA)),
             ("mle2_count_1", lambda: ops.fit_spots_mle2(alone, one, guess, sigma0=SIGMA)),
             ("mle_on_the_pairs", lambda: ops.fit_spots_mle(patches, sigma0=SIGMA)),
             ("mle_alone", lambda: ops.fit_spots_mle(alone, sigma0=SIGMA)))
    for name, fit in calls:
        what = f"{name} {n} x {P}"
        first, again = checked(what, fit), checked(what, fit)
        out[f"{name}_two_runs_bitwise_equal"] = same(first, again)
        out[f"{name}_converged"] = float((first[3] == 0).double().mean())
        out[f"{name}_mean_iterations"] = float(first[4].double().mean())
        t = checked(what, lambda: t_events(fit))
        out[f"{name}_ms"], out[f"{name}_fits_per_s"] = 1e3 * t, n / t
    out["mle2_pairs_over_mle_time"] = out["mle2_pairs_ms"] / out["mle_on_the_pairs_ms"]
    return out


def same(a, b):
    return all(bool(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y))
               for x, y in zip(a, b))


def bench(n, P):
    patches = checked("patches", lambda: poisson_patches(n, P))
    out = {"N": n, "P": P}
    for name, fs in (("mle_free_sigma", True), ("mle_fixed_sigma", False)):
        what = f"{name} {n} x {P}"
        fit = lambda: ops.fit_spots_mle(patches, sigma0=SIGMA, fit_sigma=fs)                                # noqa: E731
        first, again = checked(what, fit), checked(what, fit)
        out[f"{name}_two_runs_bitwise_equal"] = same(first, again)
        out[f"{name}_converged"] = float((first[3] == 0).double().mean())
        out[f"{name}_mean_iterations"] = float(first[4].double().mean())
        out[f"{name}_max_iterations"] = int(first[4].max())
        t = checked(what, lambda: t_events(fit))
        out[f"{name}_ms"], out[f"{name}_fits_per_s"] = 1e3 * t, n / t
    what = f"lsq {n} x {P}"
    lsq = lambda: ops.refine_gaussian(patches)                                                                # noqa: E731
    first, again = checked(what, lsq), checked(what, lsq)
    out["lsq_two_runs_bitwise_equal"] = same(first, again)
    out["lsq_converged"] = float((first[2] == 0).double().mean())
    t = checked(what, lambda: t_events(lsq))
    out["lsq_ms"], out["lsq_fits_per_s"] = 1e3 * t, n / t
    out["mle_free_sigma_over_lsq_time"] = out["mle_free_sigma_ms"] / out["lsq_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--pairs", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_localization.py needs a GPU")
    out = []
    sizes = [1000] if args.small_only else [1000, 10000, 100000] if args.pairs else [1000, 100000, 1000000]
    for n in sizes:
        for P in (7, 9):
            out.append(bench_pairs(n, P) if args.pairs else bench(n, P))
            print(json.dumps(out[-1]), flush=True)
    bad = [(o["N"], o["P"], k) for o in out for k, v in o.items() if k.endswith("_two_runs_bitwise_equal") and not v]
    if bad:
        print(f"bench_localization: two runs differ: {bad}", file=sys.stderr, flush=True)
        sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
