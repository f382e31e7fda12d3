"""Wall time of the Denoising experiment's RL-TV deconvolution (snapshots after iterations 2, 5, 10 with
create_gaussian_psf(sigma=1), tv_weight 0.01) on the CPU (the numpy restatement in helpers/generation.py, vectorised over
frames) and on the GPU (csrc/deconv.hip through ops.rl_tv_deconvolve, device tensor in -> device tensor out, ending in a
device synchronise), for one training cycle's 7 680 frames (4 D values x 64 trajectories x 30 frames) and the validation
set's 6 000 (4 x 50 x 30); the Gaussian filter kernel on the same 7 680 frames; plus one whole trajs_to_vid_norm_rl cycle
(4 x 64 trajectories -> (64, 7, 30, 9, 9) each) from numpy on the CPU and from a CUDA tensor on the GPU.
Kernel time alone: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_denoise.py --gpu-only`.

    python scripts/bench_denoise.py [--gpu-only] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch

from denoise_common import frames_9x9
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.experiments.Denoising import trainSettingsMult as S

PSF = gen.create_gaussian_psf(sigma=1)
ITS = S.RL_iterations


def t_cpu(x):
    t0 = time.perf_counter()
    gen.apply_rl_tv_tensor_iter_list(x, PSF, ITS)
    return time.perf_counter() - t0


def t_gpu(fn, reps=10):
    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    once()                                                   # first launch: code object load
    return min(once() for _ in range(reps))


def t_cycle(device, N=64, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for Ds in ([1, 1], [3, 1], [5, 1], [7, 1]):               # trainModels_different_settings.run_training.make_batch_data
        trajs, _ = gen.brownian_single_state(N, S.T, Ds=Ds, alphas=1, generator=g, device=device)
        trajs = trajs.permute(1, 0, 2) / S.traj_div_factor
        if device == "cpu":
            trajs = trajs.numpy()
        gen.trajs_to_vid_norm_rl(trajs, S.nPosPerFrame, S.center, S.image_props, ITS, generator=g)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {}
    for label, n_seq in (("cycle_7680", 4 * 64), ("validation_6000", 4 * 50)):
        x = frames_9x9(n_seq * S.nFrames, seed=1).reshape(n_seq, S.nFrames, 9, 9)
        xd = torch.as_tensor(x).cuda()
        res[f"rl_tv_{label}_gpu_ms"] = 1e3 * t_gpu(lambda: ops.rl_tv_deconvolve(xd, PSF, ITS, 0.01))
        if not a.gpu_only:
            res[f"rl_tv_{label}_cpu_ms"] = 1e3 * t_cpu(x)
    xd = torch.as_tensor(frames_9x9(7680, seed=2)).cuda()
    res["gaussian_filter_7680_gpu_ms"] = 1e3 * t_gpu(lambda: ops.gaussian_filter_frames(xd, 0.5))
    t_cycle("cuda")                                           # warm-up: renderer + deconvolution code objects
    res["trajs_to_vid_norm_rl_cycle_gpu_ms"] = 1e3 * min(t_cycle("cuda", seed=s) for s in range(3))
    if not a.gpu_only:
        res["trajs_to_vid_norm_rl_cycle_cpu_ms"] = 1e3 * t_cycle("cpu")
    for k, v in res.items():
        print(f"{k:40s} {v:10.3f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
