"""Time of the directed-motion kernel (helpers/msd.estimate_directed_ml -> ops.track_directed_ml -> csrc/directed_ml.hip)
beside the maximum-likelihood D kernel (ops.track_diffusion_ml, csrc/likelihood.hip) on the same tracks in the same process:
the track sets of bench_likelihood.py (10^3, 10^4 and 10^5 tracks of 100 rows, R = 1/6, D = 0.01, row variances 0.04 * {0.25
or 1.75}), once as they are (free walks) and once with a velocity of 0.3 pixels per unit of dt in a seeded direction per
track.  Its method too: events on the stream after a warm-up; every timed window repeats its call until it holds at least 0.2 s
of work, and the minimum of 5 windows is reported per call.  Also reported: the share of fits with status 0, the RMS pull of
the velocity components against the truth, the share of tracks with p_brownian < 0.05 on either set, and whether two runs
agree bit for bit; at the smallest size the kernel is held against the numpy restatement.  Every GPU step is followed by a
synchronisation and an error check of its own; the first error ends the script with a non-zero status.

    python scripts/bench_directed_ml.py [--small-only] [--json OUT]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bench_likelihood as bl
from bench_likelihood import DT, R, ROWS, checked, same, t_events
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import msd

SPEED = 0.3


def bench(n, verify):
    pos, var, offsets = checked("tracks", lambda: bl.tracks(n))
    g = torch.Generator(device="cuda").manual_seed(1)
    phi = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * (2.0 * math.pi)
    vel = SPEED * torch.stack([torch.sin(phi), torch.cos(phi)], dim=1)
    t = torch.arange(ROWS, device="cuda", dtype=torch.float64) * DT
    moved = (pos.view(n, ROWS, 2) + vel.view(n, 1, 2) * t.view(1, ROWS, 1)).reshape(-1, 2).contiguous()
    out = {"n_tracks": n, "rows": ROWS, "speed": SPEED}
    calls = (("ml", lambda: ops.track_diffusion_ml(pos, offsets, var, dt=DT, blur=R)),
             ("directed_free", lambda: ops.track_directed_ml(pos, offsets, var, dt=DT, blur=R)),
             ("directed", lambda: ops.track_directed_ml(moved, offsets, var, dt=DT, blur=R)))
    for name, call in calls:
        what = f"{name} {n} x {ROWS}"
        first, again = checked(what, call), checked(what, call)
        out[f"{name}_two_runs_bitwise_equal"] = same(first, again)
        out[f"{name}_status_0"] = float((first[-1] == 0).double().mean())
        if name != "ml":
            truth = vel if name == "directed" else torch.zeros_like(vel)
            fine = first[-1] == 0
            out[f"{name}_rms_pull_velocity"] = float((((first[2] - truth) / first[3])[fine]).pow(2).mean().sqrt())
            x = moved if name == "directed" else pos
            fit = checked(what, lambda: msd.estimate_directed_ml(x, offsets.long(), var, dt=DT, blur=R))
            out[f"{name}_share_p_below_0.05"] = float((fit["p_brownian"][fine] < 0.05).double().mean())
        if name == "directed" and verify:
            want = msd._directed_ml_numpy(moved.cpu().numpy(), var.cpu().numpy(), None, None, offsets.cpu().numpy().astype(np.int64), DT, R)
            got = [f.cpu().numpy() for f in first]
            out["directed_status_equals_restatement"] = bool(np.array_equal(got[6], want[6]) and np.array_equal(got[5], want[5]))
            out["directed_D_worst_relative_difference"] = float(np.nanmax(np.abs(got[0] / want[0] - 1.0)))
            out["directed_velocity_worst_difference_in_std"] = float(np.nanmax(np.abs(got[2] - want[2]) / want[3]))
        out[f"{name}_ms"] = 1e3 * checked(what, lambda: t_events(call))
    out["directed_tracks_per_s"] = n / (out["directed_ms"] * 1e-3)
    out["directed_ns_per_row_pass_candidate"] = out["directed_ms"] * 1e6 / (n * ROWS * 9 * 64)
    out["directed_over_ml_time"] = out["directed_ms"] / out["ml_ms"]
    out["directed_free_over_ml_time"] = out["directed_free_ms"] / out["ml_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_directed_ml.py needs a GPU")
    out = []
    for n in [1000] if args.small_only else [1000, 10000, 100000]:
        out.append(bench(n, verify=n == 1000))
        print(json.dumps(out[-1]), flush=True)
    bad = [(o["n_tracks"], k) for o in out for k, v in o.items() if k.endswith("_two_runs_bitwise_equal") and not v]
    if bad:
        print(f"bench_directed_ml: two runs differ: {bad}", file=sys.stderr, flush=True)
        sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
