"""Wall time of the 25 trajectory descriptors (helpers/features.py, ImagesFeatures' feature_device) on the CPU (scipy
loop) and on the GPU (csrc/features.hip through ops.trajectory_features, host array in -> features on the device, ending
in a device synchronise), for one cycle's 320 and the validation's 700 trajectories of 300 sub-steps / 30 frames and for
16 384 trajectories; plus one ImagesFeatures make_batch_data cycle (5 x 64 trajectories -> videos + features) both ways.
Kernel time alone: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_features.py --gpu-only`.

    python scripts/bench_features.py [--gpu-only] [--cpu-cap 2048] [--json OUT]
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import features as ft
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.experiments.ImagesFeatures import trainSettingsImagesFeatures as S


def walks(n, seed=0):
    return (np.cumsum(np.random.default_rng(seed).normal(size=(n, S.T, 2)), axis=1) / S.traj_div_factor).astype(np.float32)


def t_cpu(tr):
    t0 = time.perf_counter()
    ft.compute_features_for_trajectories(tr, S.nPosPerFrame, rng=np.random.default_rng(0))
    return time.perf_counter() - t0


def t_gpu(tr, reps=5):
    def once():
        t0 = time.perf_counter()
        ops.trajectory_features(torch.as_tensor(tr).cuda(), S.nPosPerFrame)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    once()                                                   # first launch: code object load
    return min(once() for _ in range(reps))


def t_cycle(feature_device, N=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    t0 = time.perf_counter()
    for Ds in ([1, 1], [3, 1], [5, 1], [7, 1], [9, 1]):       # trainModelsImagesFeatures.run_training.make_batch_data
        trajs, _ = gen.brownian_single_state(N, S.T, Ds=Ds, alphas=1, generator=g)
        S.create_video_and_feature_pairs(trajs.permute(1, 0, 2).numpy() / S.traj_div_factor, S.nPosPerFrame, S.center,
                                         S.image_props, generator=g, feature_device=feature_device)
    if feature_device:
        torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--cpu-cap", type=int, default=2048, help="largest batch timed on the CPU (larger ones: per-trajectory "
                    "time of this many, scaled; the CPU loop is linear in N)")
    ap.add_argument("--json")
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    res = {"host_cpus": len(os.sched_getaffinity(0))}
    for n in (320, 700, 16384):
        tr = walks(n)
        row = {"gpu_s": t_gpu(tr)}
        if not a.gpu_only:
            m = min(n, a.cpu_cap)
            c = t_cpu(tr[:m])
            row["cpu_s"] = c * n / m
            row["cpu_measured_on"] = m
            row["speedup"] = row["cpu_s"] / row["gpu_s"]
        res[f"N{n}"] = row
        print(f"N={n:6d}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()),
              flush=True)
    t_cycle("cuda")                                          # warm-up
    res["cycle"] = {"gpu_s": min(t_cycle("cuda", seed=s) for s in range(3))}
    if not a.gpu_only:
        res["cycle"]["cpu_s"] = t_cycle(None)
    print("make_batch_data cycle (5 x 64):", res["cycle"], flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
