"""Time of the changepoint kernels (helpers/msd.segment_tracks -> ops.segment_tracks / ops.segment_stats -> csrc/segment.hip) and
of their numpy restatement on the same input.  Events on the stream after a warm-up, minimum of 5; the restatement once, by
the wall clock.  kernel_ms is ops.segment_tracks (the launch, the allocation of its outputs and the read-back of the longest
track that sizes its LDS); stats_ms is ops.segment_stats on the segments found; call_ms is the front end, msd.segment_tracks,
from device positions and offsets to the dict.  Shapes: two-state tracks (D 0.05 / 1.0, a change every 40 rows) of a real
movie's sizes, 20 tracks of 1000 rows (the movie of scripts/bench_tracking.py), 4096 tracks of 100 rows, 352 tracks of 300
rows, and 64 tracks at the kernel's limit of ops.SEG_MAX_LEN rows.  Every GPU step is followed by a synchronisation and an
error check of its own; the first error ends the script with a non-zero status, nothing further is started.  The partition is
compared exactly with the restatement's (equal unless a margin is within rounding, which the script reports), segment_stats
bitwise.

    python scripts/bench_segment.py [--small-only] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import msd


def checked(what, fn):
    """one GPU step under its own check: run, wait for it, and leave on the first error"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as exc:                                 # noqa: BLE001  (whatever went wrong, nothing more is started)
        print(f"bench_segment: {what} failed: {exc}", file=sys.stderr, flush=True)
        sys.exit(1)


def t_events(fn, reps=5):
    fn()                                                     # warm-up: code object load, allocator
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def bench_shape(n_tracks, rows, cpu_tracks):
    rng = np.random.default_rng(0)
    D = np.where((np.arange(rows) // 40) % 2 == 0, 0.05, 1.0)
    steps = rng.standard_normal((n_tracks, rows, 2)) * np.sqrt(2.0 * D)[None, :, None]
    pos = np.ascontiguousarray(np.cumsum(steps, axis=1).reshape(-1, 2))
    offsets = np.arange(n_tracks + 1, dtype=np.int64) * rows
    dp, do = checked("upload", lambda: (torch.from_numpy(pos).cuda(), torch.from_numpy(offsets).cuda()))
    do32 = checked("upload", lambda: do.int())
    t_kernel = checked(f"kernel {n_tracks} x {rows}", lambda: t_events(lambda: ops.segment_tracks(dp, do32)))
    res = checked("front end", lambda: msd.segment_tracks(dp, do))
    so32 = checked("convert", lambda: res["seg_offsets"].int())
    end32 = checked("convert", lambda: do[res["seg_track"] + 1].int())
    t_stats = checked("stats", lambda: t_events(lambda: ops.segment_stats(dp, so32, end32)))
    t_call = checked("call", lambda: t_events(lambda: msd.segment_tracks(dp, do)))
    got = checked("download", lambda: {k: v.cpu().numpy() for k, v in res.items()})
    m = min(n_tracks, cpu_tracks)                             # the restatement is a Python loop over steps: the first m tracks
    t0 = time.perf_counter()
    start, cost, margin = msd._segment_numpy(pos[:m * rows], offsets[:m + 1], 4, 3.0, 1e-12, return_margin=True)
    t_cpu = time.perf_counter() - t0
    first = np.nonzero(start)[0]
    n_same = int(np.searchsorted(got["seg_offsets"], m * rows))
    same = len(first) == n_same and np.array_equal(got["seg_offsets"][:n_same], first)
    want = msd.segment_tracks(pos, offsets) if m == n_tracks else None
    stats_equal = None if want is None else all(np.array_equal(got[k].view(np.int64), want[k].view(np.int64))
                                                for k in ("D_cve", "D_mle", "sigma2", "n_increments"))
    return {"n_tracks": n_tracks, "rows": rows, "lds_bytes_per_workgroup": 20 * rows, "n_segments": int(len(got["seg_track"])),
            "kernel_ms": t_kernel * 1e3, "stats_ms": t_stats * 1e3, "call_ms": t_call * 1e3,
            "us_per_track": t_kernel * 1e6 / n_tracks, "cpu_restatement_tracks": m, "cpu_restatement_ms": t_cpu * 1e3,
            "partition_equal_to_restatement": bool(same), "smallest_margin": float(margin.min()),
            "worst_cost_gap": float(np.nanmax(np.abs(got["cost"][:m] - cost) / (1 + np.abs(cost)))),
            "stats_bitwise_equal_to_restatement": stats_equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment.py needs a GPU")
    shapes = [(20, 1000, 20)] if args.small_only else [(20, 1000, 20), (4096, 100, 256), (352, 300, 64), (64, ops.SEG_MAX_LEN, 2)]
    out = []
    for n_tracks, rows, cpu_tracks in shapes:
        out.append(bench_shape(n_tracks, rows, cpu_tracks))
        print(json.dumps(out[-1]), flush=True)
        if not out[-1]["partition_equal_to_restatement"] or out[-1]["stats_bitwise_equal_to_restatement"] is False:
            print("bench_segment: the kernel and the restatement differ", file=sys.stderr, flush=True)
            sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
