"""Time of the whole-field simulator (helpers/generation.render_movie -> csrc/movie.hip, and simulate_movie whole) against the
way the project made such a movie before: gpu_movie of scripts/bench_tracking.py, imported as it stands (dense torch profiles
and an einsum per 50 frames, no sub-frame motion, no up-sampled PSF, no truth).  Events on the stream after a warm-up, minimum
of 5, as bench_tracking.py times.  Two scenes, both with 10 sub-positions per frame and an up-sampling factor of 5: 30 x 128 x
128 with 12 particles and 1 000 x 512 x 512 with 50 particles.  The floor of the kernel is its one mandatory write of
F * H * W * 4 bytes; the achieved fraction of the HBM peak (--hbm-tbps, default 8.0: the MI355X's) is printed with it.

    python scripts/bench_movie_sim.py [--small-only] [--json OUT]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

import bench_tracking as bt
from moleculardiffusion_mivit_amd.helpers import generation as gen

NPOS, UP = 10, 5


def bench_scene(F, H, W, particles, hbm_tbps):
    props = dict(gen.DEFAULT_IMAGE_PROPS)
    sigma = gen.psf_sigma_hr(props)
    g = torch.Generator(device="cuda").manual_seed(0)
    _, truth = gen.simulate_movie(particles, F, H, W, 0.05, NPOS, generator=g, device="cuda")
    pos, amp = truth["pos"], truth["amp"]
    t_kernel = bt.t_events(lambda: gen.render_movie(pos, amp, sigma, H, W, UP))
    t_sim = bt.t_events(lambda: gen.simulate_movie(particles, F, H, W, 0.05, NPOS, generator=g, device="cuda"))
    t_parent = bt.t_events(lambda: bt.gpu_movie(F, H, W, particles))
    floor_bytes = F * H * W * 4
    return {"scene": f"{F} x {H} x {W}, {particles} particles, npos {NPOS}, up {UP}",
            "radius": gen.default_movie_radius(sigma, UP),
            "render_movie_ms": t_kernel * 1e3, "simulate_movie_ms": t_sim * 1e3, "gpu_movie_ms": t_parent * 1e3,
            "write_floor_bytes": floor_bytes, "write_GBps": floor_bytes / t_kernel * 1e-9,
            "fraction_of_hbm_peak": floor_bytes / t_kernel / (hbm_tbps * 1e12)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--hbm-tbps", type=float, default=8.0)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_movie_sim.py needs a GPU")
    rows = [bench_scene(30, 128, 128, 12, args.hbm_tbps)]
    if not args.small_only:
        rows.append(bench_scene(1000, 512, 512, 50, args.hbm_tbps))
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
