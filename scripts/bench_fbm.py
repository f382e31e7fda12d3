"""Time of the fractional-Gaussian-noise kernel (helpers/generation.fractional_gaussian_noise -> ops.fgn -> csrc/fbm.hip) and
of its numpy restatement on the same input.  Events on the stream after a warm-up, minimum of 5; the restatement once, by the
wall clock.  Shapes, all with C = 2 axes and exponents drawn per trajectory from 16 values: N = 352 / T = 300 (one training
cycle's refresh in the reference's loops), N = 4096 / T = 300 and N = 4096 / T = 2048 (the kernel's limit).  The restatement
costs O(N T^2) in numpy passes; at the largest shape it runs on the first --cpu-rows trajectories (default 256) and the time is
reported for those.  gamma_ms is the host side of a call: torch.unique and the autocovariance rows, included in call_ms.

    python scripts/bench_fbm.py [--small-only] [--cpu-rows 256] [--json OUT]
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
from moleculardiffusion_mivit_amd.helpers import generation as gen


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


def bench_shape(N, T, C, cpu_rows):
    rng = np.random.default_rng(0)
    alphas = rng.choice(np.linspace(gen.ALPHA_MIN, gen.ALPHA_MAX, 16), size=N)
    z = rng.standard_normal((N, T, C))
    zd, ad = torch.from_numpy(z).cuda(), torch.from_numpy(alphas)
    uniq, inv = torch.unique(ad, return_inverse=True)
    gamma = torch.from_numpy(gen.fgn_autocovariance(uniq.numpy(), T)).cuda()
    rows = inv.int().cuda()
    t_kernel = t_events(lambda: ops.fgn(zd, gamma, rows))
    t_call = t_events(lambda: gen.fractional_gaussian_noise(zd, ad))
    got = gen.fractional_gaussian_noise(zd, ad).cpu().numpy()
    n_cpu = min(N, cpu_rows)
    t0 = time.perf_counter()
    want = gen.fractional_gaussian_noise(z[:n_cpu], alphas[:n_cpu])
    t_cpu = time.perf_counter() - t0
    # what the recursion needs: per step n and axis two multiply-adds over n terms, plus the shared sum and the phi update
    flops = N * T * T / 2 * (2 + 4 * C + 2 * 2)
    return {"N": N, "T": T, "C": C, "kernel_ms": t_kernel * 1e3, "call_ms": t_call * 1e3,
            "us_per_step": t_kernel * 1e6 / T, "fp64_gflops": flops / t_kernel * 1e-9,
            "lds_bytes_per_workgroup": ((2 + C) * T + 4 * (1 + 2 * C)) * 8,
            "cpu_rows": n_cpu, "cpu_restatement_ms": t_cpu * 1e3, "cpu_ms_per_trajectory": t_cpu * 1e3 / n_cpu,
            "max_abs_kernel_minus_restatement": float(np.abs(got[:n_cpu] - want).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--cpu-rows", type=int, default=256)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fbm.py needs a GPU")
    shapes = [(352, 300, 2)] if args.small_only else [(352, 300, 2), (4096, 300, 2), (4096, ops.FGN_MAX_T, 2)]
    out = []
    for N, T, C in shapes:
        out.append(bench_shape(N, T, C, N if T <= 300 else args.cpu_rows))
        print(json.dumps(out[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
