"""Time of the run-and-pause segmenter (ops.segment_transport) next to the variance-change segmenter whose recurrence kernel
it shares (ops.segment_tracks; both csrc/segment.hip), in ONE process on the same input: the track sets of
scripts/bench_segment.py (two-state tracks, D 0.05 / 1.0, a change every 40 rows: 20 tracks of 1000 rows, 4096 of 100, 352 of
300, and 64 at the limit of 4096 rows).
Events on the stream after a warm-up, minimum of 5 windows.  Each time is the ops call: the launch, the allocation of its
outputs and the read-back of the longest track that sizes its LDS.  segment_transport is timed in its three modes; "both" and
"directed" take two logs per candidate where segment_tracks takes one, "diffusive" takes one and must reproduce
segment_tracks bit for bit, which the script checks; stats_ms is ops.transport_stats on the stretches that "both" found.
Every GPU step is followed by a synchronisation and an error check of its own; the first error ends the script with a non-zero
status, nothing further is started.

    python scripts/bench_transport.py [--small-only] [--json OUT]
"""
import argparse
import json
import os
import sys

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
        print(f"bench_transport: {what} failed: {exc}", file=sys.stderr, flush=True)
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


def bench_shape(n_tracks, rows):
    rng = np.random.default_rng(0)                           # the tracks of scripts/bench_segment.py
    D = np.where((np.arange(rows) // 40) % 2 == 0, 0.05, 1.0)
    steps = rng.standard_normal((n_tracks, rows, 2)) * np.sqrt(2.0 * D)[None, :, None]
    pos = np.ascontiguousarray(np.cumsum(steps, axis=1).reshape(-1, 2))
    offsets = np.arange(n_tracks + 1, dtype=np.int64) * rows
    dp, do = checked("upload", lambda: (torch.from_numpy(pos).cuda(), torch.from_numpy(offsets).cuda()))
    do32 = checked("upload", lambda: do.int())
    out = {"n_tracks": n_tracks, "rows": rows, "lds_bytes_segment_tracks": 20 * rows,           # "diffusive" runs its kernel
           "lds_bytes_segment_transport": {"both": 36 * rows, "directed": 36 * rows, "diffusive": 20 * rows}}
    t_seg = checked(f"segment_tracks {n_tracks} x {rows}", lambda: t_events(lambda: ops.segment_tracks(dp, do32)))
    out["segment_tracks_ms"] = t_seg * 1e3
    for mode in ("both", "directed", "diffusive"):
        t = checked(f"segment_transport {mode} {n_tracks} x {rows}",
                    lambda: t_events(lambda: ops.segment_transport(dp, do32, classes=mode)))
        out[f"transport_{mode}_ms"] = t * 1e3
        out[f"ratio_{mode}"] = t / t_seg
    ref = checked("segment_tracks", lambda: ops.segment_tracks(dp, do32))
    dif = checked("segment_transport diffusive", lambda: ops.segment_transport(dp, do32, classes="diffusive"))
    out["diffusive_equals_segment_tracks"] = bool(torch.equal(ref[0], dif[0])) and bool(
        torch.equal(ref[1].view(torch.int64), dif[2].view(torch.int64)))
    res = checked("front end", lambda: msd.segment_transport(dp, do))
    so32 = checked("convert", lambda: res["seg_offsets"].int())
    end32 = checked("convert", lambda: do[res["seg_track"] + 1].int())
    out["stats_ms"] = checked("stats", lambda: t_events(lambda: ops.transport_stats(dp, so32, end32))) * 1e3
    out["n_stretches"] = int(len(res["seg_track"]))
    out["n_directed_stretches"] = int(res["seg_class"].sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transport.py needs a GPU")
    shapes = [(20, 1000)] if args.small_only else [(20, 1000), (4096, 100), (352, 300), (64, ops.TRANSPORT_MAX_LEN)]
    out = []
    for n_tracks, rows in shapes:
        out.append(bench_shape(n_tracks, rows))
        print(json.dumps(out[-1]), flush=True)
        if not out[-1]["diffusive_equals_segment_tracks"]:
            print("bench_transport: the diffusive mode and segment_tracks differ", file=sys.stderr, flush=True)
            sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
