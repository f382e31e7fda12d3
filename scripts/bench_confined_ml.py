"""Time of the maximum-likelihood confinement kernel (helpers/msd.estimate_confinement_ml -> ops.track_confined_ml ->
csrc/confined_ml.hip) on 10^3, 10^4 and 10^5 tracks of 100 rows, with ops.track_confined_loglik (one evaluation a track) and
ops.track_diffusion_ml (csrc/likelihood.hip, blur 0) on the same batch as controls, and at the smallest size the numpy
restatement (helpers/msd._confined_ml_numpy) on the CPU, against which the kernel is also held.  The tracks are drawn from
the model on the GPU: D = 0.5, lambda = 0.6, dt = 0.5, row variances 0.02 * {0.25 or 1.75} per row and axis, started in the
stationary law.  The method of bench_likelihood.py: events on the stream after a warm-up; every timed window repeats its
call until it holds at least 0.2 s of work, and the minimum of 5 windows is reported per call (the outputs are allocated
inside the call, as a user's are).  Also reported: the share of fits with status 0, the median radius and D, the RMS pull of
ln D_conf, and whether two runs agree bit for bit.  Every GPU step is followed by a synchronisation and an error check of its
own; the first error ends the script with a non-zero status, nothing further is started.

    python scripts/bench_confined_ml.py [--small-only] [--json OUT]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import msd

ROWS, D, LAM, V0, DT = 100, 0.5, 0.6, 0.02, 0.5
S2 = D / LAM
PASSES = 23                  # csrc/confined_ml.hip: two for the reference scales, 20 rounds, one for the stencil


def checked(what, fn):
    """one GPU step under its own check: run, wait for it, and leave on the first error"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as exc:                                 # noqa: BLE001  (whatever went wrong, nothing more is started)
        print(f"bench_confined_ml: {what} failed: {exc}", file=sys.stderr, flush=True)
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


def tracks(n, seed=0):
    """(pos [n * ROWS, 2], var [n * ROWS, 2] float64, offsets [n + 1] int32) on the GPU, drawn there: the exact discretisation
    of the Ornstein-Uhlenbeck process about (30, 30), plus the row's noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(n, ROWS, 2, generator=g, device="cuda", dtype=torch.float64)
    phi = math.exp(-LAM * DT)
    x = torch.empty_like(z)
    x[:, 0] = z[:, 0] * S2 ** 0.5
    for k in range(1, ROWS):
        x[:, k] = phi * x[:, k - 1] + (S2 * (1.0 - phi * phi)) ** 0.5 * z[:, k]
    var = V0 * torch.where(torch.rand(n, ROWS, 2, generator=g, device="cuda") < 0.5, 0.25, 1.75).double()
    pos = 30.0 + x + torch.randn(n, ROWS, 2, generator=g, device="cuda", dtype=torch.float64) * var.sqrt()
    offsets = torch.arange(n + 1, device="cuda", dtype=torch.int32) * ROWS
    return pos.reshape(-1, 2).contiguous(), var.reshape(-1, 2).contiguous(), offsets


def same(a, b):
    return all(bool(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y))
               for x, y in zip(a, b))


def bench(n, verify):
    pos, var, offsets = checked("tracks", lambda: tracks(n))
    Dn, Sn = (torch.full((n,), v, dtype=torch.float64, device="cuda") for v in (D, S2))
    out = {"n_tracks": n, "rows": ROWS}
    calls = (("confined_ml", lambda: ops.track_confined_ml(pos, offsets, var, dt=DT)),
             ("confined_loglik", lambda: (ops.track_confined_loglik(pos, offsets, Dn, Sn, None, var, dt=DT),)),
             ("diffusion_ml", lambda: ops.track_diffusion_ml(pos, offsets, var, dt=DT, blur=0.0)))
    for name, call in calls:
        what = f"{name} {n} x {ROWS}"
        first, again = checked(what, call), checked(what, call)
        out[f"{name}_two_runs_bitwise_equal"] = same(first, again)
        if name == "confined_ml":
            fit = dict(zip(msd._CF_OUTS, first))
            fine = fit["status"] == 0
            out["status_0"] = float(fine.double().mean())
            out["radius_median"], out["radius_true"] = float(fit["radius"][fine].median()), (2.0 * S2) ** 0.5
            out["D_conf_median"] = float(fit["D_conf"][fine].median())
            out["rms_pull_ln_D"] = float(((torch.log(fit["D_conf"] / D) / (fit["D_conf_std"] / fit["D_conf"]))[fine]).pow(2).mean().sqrt())
            pull = (torch.log(fit["radius"] / out["radius_true"]) / (fit["radius_std"] / fit["radius"]))[fine]
            out["mean_pull_ln_radius"], out["rms_pull_ln_radius"] = float(pull.mean()), float(pull.pow(2).mean().sqrt())
            if verify:
                args = (pos.cpu().numpy(), var.cpu().numpy(), None, None, offsets.cpu().numpy().astype(np.int64), DT)
                t0 = time.perf_counter()
                want = dict(zip(msd._CF_OUTS, msd._confined_ml_numpy(*args)))
                out["restatement_cpu_ms"] = 1e3 * (time.perf_counter() - t0)
                got = {k: v.cpu().numpy() for k, v in fit.items()}
                out["status_equals_restatement"] = bool(np.array_equal(got["status"], want["status"]) and np.array_equal(got["n_increments"], want["n_increments"]))
                out["radius_worst_relative_difference"] = float(np.nanmax(np.abs(got["radius"] / want["radius"] - 1.0)))
                out["loglik_worst_relative_difference"] = float(np.nanmax(np.abs(got["loglik"] / want["loglik"] - 1.0)))
        t = checked(what, lambda: t_events(call))
        out[f"{name}_ms"] = 1e3 * t
    out["confined_ml_tracks_per_s"] = n / (out["confined_ml_ms"] * 1e-3)
    out["confined_ml_us_per_track"] = out["confined_ml_ms"] * 1e3 / n
    out["confined_ml_ns_per_row_pass_candidate"] = out["confined_ml_ms"] * 1e6 / (n * ROWS * PASSES * 64)
    out["confined_ml_over_diffusion_ml_time"] = out["confined_ml_ms"] / out["diffusion_ml_ms"]
    if "restatement_cpu_ms" in out:
        out["restatement_over_confined_ml_time"] = out["restatement_cpu_ms"] / out["confined_ml_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_confined_ml.py needs a GPU")
    out = []
    for n in [1000] if args.small_only else [1000, 10000, 100000]:
        out.append(bench(n, verify=n == 1000))
        print(json.dumps(out[-1]), flush=True)
    bad = [(o["n_tracks"], k) for o in out for k, v in o.items() if k.endswith("_two_runs_bitwise_equal") and not v]
    if bad:
        print(f"bench_confined_ml: two runs differ: {bad}", file=sys.stderr, flush=True)
        sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
