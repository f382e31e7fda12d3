"""Time of the maximum-likelihood anomalous-exponent kernel (helpers/msd.estimate_anomalous_ml -> ops.track_fbm_ml ->
csrc/fbm_ml.hip) on 10^2, 10^3 and 10^4 tracks of 100 rows, with ops.track_fbm_loglik (one evaluation of the likelihood a
track), ops.track_diffusion_ml (csrc/likelihood.hip) and ops.track_msd + helpers/msd.estimate_alpha (the slope of the MSD) on
the same tracks for scale.  The tracks are those of bench_likelihood.py: Brownian (alpha = 1), exposure over the whole frame,
D = 0.01, row variances 0.04 * {0.25 or 1.75} per row and axis.  The method is bench_likelihood.py's: events on the stream
after a warm-up; every timed window repeats its call until it holds at least 0.2 s of work, and the minimum of 5 windows is
reported per call (the outputs and the workspace are allocated inside the call, as a user's are).  Also reported: the share
of fits with status 0, the median and the RMS pull of alpha_ml, and whether two runs agree bit for bit.  Every GPU step is
followed by a synchronisation and an error check of its own; the first error ends the script with a non-zero status, nothing
further is started.

    python scripts/bench_fbm_ml.py [--small-only] [--json OUT]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from bench_likelihood import DT, R, ROWS, same, t_events, tracks
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import msd

EXPOSURE = 1.0


def checked(what, fn):
    """one GPU step under its own check: run, wait for it, and leave on the first error"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as exc:                                 # noqa: BLE001  (whatever went wrong, nothing more is started)
        print(f"bench_fbm_ml: {what} failed: {exc}", file=sys.stderr, flush=True)
        sys.exit(1)


def bench(n):
    pos, var, offsets = checked("tracks", lambda: tracks(n))
    one = torch.ones(n, dtype=torch.float64, device="cuda")
    out = {"n_tracks": n, "rows": ROWS}
    calls = (("fbm_ml", lambda: ops.track_fbm_ml(pos, offsets, var, dt=DT, exposure=EXPOSURE)),
             ("fbm_loglik", lambda: ops.track_fbm_loglik(pos, offsets, one, 0.01 * one, var, dt=DT, exposure=EXPOSURE)),
             ("diffusion_ml", lambda: ops.track_diffusion_ml(pos, offsets, var, dt=DT, blur=R)),
             ("msd_alpha", lambda: (msd.estimate_alpha(ops.track_msd(pos, offsets, DT, 10)[0], max_lag=10),)))
    for name, call in calls:
        what = f"{name} {n} x {ROWS}"
        first, again = checked(what, call), checked(what, call)
        out[f"{name}_two_runs_bitwise_equal"] = same(first, again)
        if name == "fbm_ml":
            fine = first[7] == 0
            out["fbm_ml_status_0"] = float(fine.double().mean())
            out["alpha_ml_median"] = float(first[0][fine].median())
            out["alpha_ml_rms_pull"] = float((((first[0] - 1.0) / first[1])[fine]).pow(2).mean().sqrt())
            out["alpha_ml_rms_error"] = float((first[0] - 1.0)[fine].pow(2).mean().sqrt())
        if name == "msd_alpha":
            out["alpha_msd_median"] = float(first[0].nanmedian())
            out["alpha_msd_rms_error"] = float((first[0] - 1.0).pow(2).nanmean().sqrt())
        out[f"{name}_ms"] = 1e3 * checked(what, lambda: t_events(call))
    out["fbm_ml_tracks_per_s"] = n / (out["fbm_ml_ms"] * 1e-3)
    out["fbm_ml_us_per_factorisation"] = out["fbm_ml_ms"] * 1e3 / (n * (20 * 64 + 9) * 2)
    out["fbm_ml_over_diffusion_ml_time"] = out["fbm_ml_ms"] / out["diffusion_ml_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fbm_ml.py needs a GPU")
    out = []
    for n in [100] if args.small_only else [100, 1000, 10000]:
        out.append(bench(n))
        print(json.dumps(out[-1]), flush=True)
    bad = [(o["n_tracks"], k) for o in out for k, v in o.items() if k.endswith("_two_runs_bitwise_equal") and not v]
    if bad:
        print(f"bench_fbm_ml: two runs differ: {bad}", file=sys.stderr, flush=True)
        sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
