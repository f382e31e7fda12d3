"""Time of the hidden-Markov kernels (helpers/msd.fit_diffusion_states -> ops.hmm_estep / ops.hmm_viterbi -> csrc/hmm.hip) and
of their numpy restatement on the same input.  Events on the stream after a warm-up, minimum of 5; the restatement once, by
the wall clock.  estep_ms is ops.hmm_estep (the launch, the allocation of its outputs and workspace and the check of the
offsets on the host), viterbi_ms is ops.hmm_viterbi likewise (with the three logarithms taken in torch), fit_ms a whole
msd.fit_diffusion_states from the default start (n_iter E-steps, reported), cpu_estep_ms one E-step of the restatement.
Shapes: two-state tracks (D 0.05 / 1.0, a change every 40 rows), 4096 tracks of 100 rows, 352 of 300, 20 of 1000 and 64 of
4096, each for K = 2, 3 and 8.  Every GPU step is followed by a synchronisation and an error check of its own; the first
error ends the script with a non-zero status, nothing further is started.  The E-step is compared with the restatement
(largest error of gamma, absolute, and of the statistics, relative to 1 + |x|), the Viterbi path and its log-probability
bit for bit.

    python scripts/bench_hmm.py [--small-only] [--json OUT]
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
        print(f"bench_hmm: {what} failed: {exc}", file=sys.stderr, flush=True)
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


def parameters(K):
    v = np.geomspace(0.1, 2.0, K) if K > 1 else np.array([1.0])
    A = np.full((K, K), 0.1 / max(K - 1, 1)) + np.eye(K) * (0.9 - 0.1 / max(K - 1, 1)) if K > 1 else np.ones((1, 1))
    return v, A, np.full(K, 1.0 / K)


def bench_shape(n_tracks, rows, K):
    rng = np.random.default_rng(0)
    D = np.where((np.arange(rows) // 40) % 2 == 0, 0.05, 1.0)
    steps = rng.standard_normal((n_tracks, rows, 2)) * np.sqrt(2.0 * D)[None, :, None]
    pos = np.ascontiguousarray(np.cumsum(steps, axis=1).reshape(-1, 2))
    offsets = np.arange(n_tracks + 1, dtype=np.int64) * rows
    v, A, pi = parameters(K)
    dp, do = checked("upload", lambda: (torch.from_numpy(pos).cuda(), torch.from_numpy(offsets).cuda()))
    do32, dv, dA, dpi = checked("upload", lambda: (do.int(), torch.from_numpy(v).cuda(), torch.from_numpy(A).cuda(),
                                                   torch.from_numpy(pi).cuda()))
    t_estep = checked(f"E-step {n_tracks} x {rows}, K = {K}", lambda: t_events(lambda: ops.hmm_estep(dp, do32, dv, dA, dpi)))
    t_vit = checked(f"Viterbi {n_tracks} x {rows}, K = {K}", lambda: t_events(lambda: ops.hmm_viterbi(dp, do32, dv, dA, dpi)))
    fit = checked("fit", lambda: msd.fit_diffusion_states(dp, do, K))
    t_fit = checked("fit", lambda: t_events(lambda: msd.fit_diffusion_states(dp, do, K), reps=2))
    got = checked("download", lambda: [o.cpu().numpy() for o in ops.hmm_estep(dp, do32, dv, dA, dpi)])
    path, logp = checked("download", lambda: [o.cpu().numpy() for o in ops.hmm_viterbi(dp, do32, dv, dA, dpi)])
    logs = checked("logs", lambda: [torch.log(t).cpu().numpy() for t in (dv, dA, dpi)])
    t0 = time.perf_counter()
    want = msd._hmm_estep_numpy(pos, offsets, v, A, pi)
    t_cpu = time.perf_counter() - t0
    want_path, want_logp = msd._hmm_viterbi_numpy(pos, offsets, v, *logs)
    gamma_err = float(np.abs(got[0] - want[0]).max())
    stat_err = max(float((np.abs(g - w) / (1.0 + np.abs(w))).max()) for g, w in zip(got[2:], want[2:]))
    return {"n_tracks": n_tracks, "rows": rows, "K": K, "estep_ms": t_estep * 1e3, "viterbi_ms": t_vit * 1e3,
            "fit_ms": t_fit * 1e3, "fit_n_iter": fit["n_iter"], "fit_Ds": [float(d) for d in fit["Ds"]],
            "ns_per_increment_estep": t_estep * 1e9 / (n_tracks * (rows - 1)), "cpu_estep_ms": t_cpu * 1e3,
            "gamma_max_abs_err": gamma_err, "stats_max_rel_err": stat_err,
            "viterbi_bitwise_equal_to_restatement": bool(np.array_equal(path, want_path) and
                                                         np.array_equal(logp.view(np.int64), want_logp.view(np.int64)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hmm.py needs a GPU")
    shapes = [(20, 1000)] if args.small_only else [(4096, 100), (352, 300), (20, 1000), (64, 4096)]
    out = []
    for n_tracks, rows in shapes:
        for K in (2, 3, 8):
            out.append(bench_shape(n_tracks, rows, K))
            print(json.dumps(out[-1]), flush=True)
            if not out[-1]["viterbi_bitwise_equal_to_restatement"] or out[-1]["gamma_max_abs_err"] > 1e-10:
                print("bench_hmm: the kernel and the restatement differ", file=sys.stderr, flush=True)
                sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
