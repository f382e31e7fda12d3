"""Time of the drift kernels (helpers/msd.estimate_drift -> ops.drift_frames / ops.drift_integrate -> csrc/drift.hip) in both
estimators, and of the torch composition a user would write instead, on the same GPU and the same input: for the mean
index_add_ over the frames + a division + cumsum (atomics: not repeatable run to run), for the median a loop of torch.median
over the frames + cumsum (torch.median returns the LOWER middle value of an even count, so it is not the same number; it is
the time that is compared).  Events on the stream after a warm-up; every timed window repeats its call until it holds at
least 0.2 s of work, and the minimum of 5 windows is reported per call.  frames_ms is ops.drift_frames alone (the launch, the
allocation of its output and the read-back of frame_offsets for the checks), integrate_ms ops.drift_integrate alone,
estimate_ms a whole msd.estimate_drift (the pair list in torch included), torch_ms the composition from the same pair list.
Shapes: movies of 1000 frames with 20, 352 and 4096 tracks that live through the movie (the track counts of bench_hmm.py;
4096 pairs a frame is the median's limit), and the running sum alone at F = 100 000.  Every GPU step is followed by a
synchronisation and an error check of its own; the first error ends the script with a non-zero status, nothing further is
started.  The kernels are compared with the numpy restatements bit for bit, and two runs of each with each other.

    python scripts/bench_drift.py [--small-only] [--json OUT]
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
        print(f"bench_drift: {what} failed: {exc}", file=sys.stderr, flush=True)
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


def torch_mean(pos, rows, pf, F):
    d = pos[rows] - pos[rows - 1]
    s = torch.zeros(F, 2, dtype=torch.float64, device=pos.device).index_add_(0, pf, d)
    n = torch.bincount(pf, minlength=F)
    v = torch.where(n[:, None] > 0, s / n.clamp(min=1)[:, None], torch.zeros((), dtype=torch.float64, device=pos.device))
    return torch.cumsum(v, 0)


def torch_median(pos, rows, bounds, F):
    d = pos[rows] - pos[rows - 1]
    v = torch.zeros(F, 2, dtype=torch.float64, device=pos.device)
    for f in range(F):                                       # bounds: the frame offsets on the host
        if bounds[f + 1] > bounds[f]:
            v[f] = torch.median(d[bounds[f]:bounds[f + 1]], dim=0).values
    return torch.cumsum(v, 0)


def bits(t):
    return t.cpu().numpy().view(np.int64)


def bench_movie(n_tracks, F):
    rng = np.random.default_rng(0)
    steps = rng.standard_normal((n_tracks, F, 2)) * np.sqrt(2.0 * 0.05) + np.array([0.0, 0.3])
    pos = np.ascontiguousarray(np.cumsum(steps, axis=1).reshape(-1, 2))
    frames = np.tile(np.arange(F, dtype=np.int64), n_tracks)
    offsets = np.arange(n_tracks + 1, dtype=np.int64) * F
    dp, df, do = checked("upload", lambda: tuple(torch.from_numpy(a).cuda() for a in (pos, frames, offsets)))
    rows, counts, fo, _ = checked("pair list", lambda: msd._drift_pairs(dp, df, do, None, F, 1))
    rows32, fo32, n32, pf = checked("pair list", lambda: (rows.int(), fo.int(), counts.int(), df[rows]))
    bounds = fo.cpu().tolist()
    out = {"n_tracks": n_tracks, "frames": F, "pairs": int(rows.numel())}
    for mode in ("mean", "median"):
        what = f"{mode} {n_tracks} x {F}"
        stat = checked(what, lambda: ops.drift_frames(dp, rows32, fo32, mode))
        again = checked(what, lambda: ops.drift_frames(dp, rows32, fo32, mode))
        vel, drift = checked(what, lambda: ops.drift_integrate(stat, n32, 0))
        want = msd._drift_frames_numpy(pos, rows.cpu().numpy(), fo.cpu().numpy(), ops.DRIFT_MODES[mode])
        want_vel, want_drift = msd._drift_integrate_numpy(want, counts.cpu().numpy(), 0)
        out[f"{mode}_bitwise_equal_to_restatement"] = bool(
            np.array_equal(bits(stat), want.view(np.int64)) and np.array_equal(bits(vel), want_vel.view(np.int64))
            and np.array_equal(bits(drift), want_drift.view(np.int64)))
        out[f"{mode}_two_runs_bitwise_equal"] = bool(np.array_equal(bits(stat), bits(again)))
        out[f"{mode}_frames_ms"] = 1e3 * checked(what, lambda: t_events(lambda: ops.drift_frames(dp, rows32, fo32, mode)))
        out[f"{mode}_estimate_ms"] = 1e3 * checked(what, lambda: t_events(lambda: msd.estimate_drift(dp, df, do, estimator=mode)))
        if mode == "mean":
            ref = checked("torch mean", lambda: torch_mean(dp, rows, pf, F))
            ref2 = checked("torch mean", lambda: torch_mean(dp, rows, pf, F))
            out["torch_mean_two_runs_bitwise_equal"] = bool(np.array_equal(bits(ref), bits(ref2)))
            out["torch_mean_ms"] = 1e3 * checked("torch mean", lambda: t_events(lambda: torch_mean(dp, rows, pf, F)))
        else:
            ref = checked("torch median", lambda: torch_median(dp, rows, bounds, F))
            out["torch_median_ms"] = 1e3 * checked("torch median",
                                                   lambda: t_events(lambda: torch_median(dp, rows, bounds, F), windows=3))
        out[f"{mode}_max_abs_diff_to_torch"] = float((ref - drift).abs().max())
    out["integrate_ms"] = 1e3 * checked("integrate", lambda: t_events(lambda: ops.drift_integrate(stat, n32, 0)))
    out["integrate_h5_ms"] = 1e3 * checked("integrate", lambda: t_events(lambda: ops.drift_integrate(stat, n32, 5)))
    return out


def bench_integrate(F):
    rng = np.random.default_rng(1)
    stat, n = rng.normal(0.1, 1.0, (F, 2)), rng.integers(1, 9, F).astype(np.int32)
    ds, dn = checked("upload", lambda: (torch.from_numpy(stat).cuda(), torch.from_numpy(n).cuda()))
    out = {"frames": F}
    for h in (0, 5):
        vel, drift = checked("integrate", lambda: ops.drift_integrate(ds, dn, h))
        wv, wd = msd._drift_integrate_numpy(stat, n, h)
        out[f"h{h}_bitwise_equal_to_restatement"] = bool(np.array_equal(bits(vel), wv.view(np.int64)) and
                                                         np.array_equal(bits(drift), wd.view(np.int64)))
        out[f"h{h}_integrate_ms"] = 1e3 * checked("integrate", lambda: t_events(lambda: ops.drift_integrate(ds, dn, h)))
    out["torch_cumsum_ms"] = 1e3 * checked("cumsum", lambda: t_events(lambda: torch.cumsum(ds, 0)))
    out["max_abs_diff_to_torch_cumsum"] = float((torch.cumsum(ds, 0)[1:] - ds[0] - ops.drift_integrate(ds, dn, 0)[1][1:]).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_drift.py needs a GPU")
    out = []
    for n_tracks in ([20] if args.small_only else [20, 352, 4096]):
        out.append(bench_movie(n_tracks, 1000))
        print(json.dumps(out[-1]), flush=True)
    out.append(bench_integrate(1000 if args.small_only else 100000))
    print(json.dumps(out[-1]), flush=True)
    bad = [k for o in out for k, v in o.items() if k.endswith("equal_to_restatement") and not v] + \
          [k for o in out for k, v in o.items() if k.endswith("_two_runs_bitwise_equal") and not k.startswith("torch") and not v]
    if bad:
        print(f"bench_drift: the kernel and the restatement differ: {bad}", file=sys.stderr, flush=True)
        sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
