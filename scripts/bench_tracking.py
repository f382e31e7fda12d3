"""Wall time of the real-movie front end (helpers/tracking.py): detection (csrc/tracking.hip through ops.dog_peaks), the
Gaussian fit (ops.refine_gaussian) and a whole track_particles_flat on the GPU, device tensor in, timed with events on the
stream after a warm-up (minimum of the repetitions; track_particles_flat ends on the host, so it is timed with the wall
clock around a synchronise); the numpy restatement; and a reference-style per-frame loop on the CPU (two
scipy.ndimage.gaussian_filter calls and the peak_local_max statement per frame, one scipy.optimize.curve_fit per patch).
Two shapes: the fixture's 30 x 128 x 128 movie with 12 particles, and 1 000 x 512 x 512 with about 50 particles per frame;
on the large one the CPU paths run on the first --cpu-frames frames and the time is reported per frame.  A third movie,
1 000 x 512 x 512 with about 200 particles, is used for the linking rows only.
Linking rows: the host loop (_link_tracks: scipy per frame), the numpy restatement of csrc/linking.hip
(link_particles_movie on host arrays, on the first --cpu-frames frames), the device (ops.link_frames + ops.chain_tracks +
the table, events), and the whole track_particles_flat with linking="host" and linking="device" (wall clock around a
synchronise, minimum of 5).  Gap closing: ops.close_gaps alone at max_gap 2 and 8 (events), and the whole
track_particles_flat(linking="device") at max_gap 0 and 2; the movies of this script have no dark frames, so the gaps closed
are the detector's own misses.
Diffusion rows (both movie sizes): the stage from the detections table to the model's input and the MSD estimates on the device
(tracks_table_by_track + refine_localizations_tensors + ops.track_msd + track_sequences; csrc/diffusion.hip) against the
host-shaped way of doing the same (extract_patches_flat + normalize_images, refine_localizations on the host, a Python loop of
helpers/msd calls per track), events, minimum of 5, and the two kernels alone.

    python scripts/bench_tracking.py [--small-only] [--cpu-frames N] [--json OUT]
"""
import argparse
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch

import tracking_common as tc
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import tracking as T

W1, W2 = T.gaussian_half_kernel(1.0), T.gaussian_half_kernel(2.0)
PATCH = tc.PATCH_SIZE


def gpu_movie(frames, H, W, particles, seed=0):
    """Gaussian spots on Brownian paths, background, Poisson noise, rendered on the device: float32 [frames, H, W]."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    start = torch.rand(1, particles, 2, generator=g, device="cuda") * torch.tensor([H - 40.0, W - 40.0], device="cuda") + 20
    pos = start + torch.cumsum(torch.randn(frames, particles, 2, generator=g, device="cuda") * 0.3, dim=0)
    out = torch.empty(frames, H, W, device="cuda")
    yy, xx = torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32)
    for f0 in range(0, frames, 50):
        p = pos[f0:f0 + 50]
        gy = torch.exp(-(yy[None, None, :] - p[:, :, 0:1]) ** 2 / (2 * 1.3 ** 2))
        gx = torch.exp(-(xx[None, None, :] - p[:, :, 1:2]) ** 2 / (2 * 1.3 ** 2))
        out[f0:f0 + 50] = torch.poisson(200.0 * torch.einsum("fpy,fpx->fyx", gy, gx) + 20.0, generator=g)
    return out


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


def t_wall(fn, reps=1):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def quiet(fn):
    def run():
        with redirect_stdout(io.StringIO()):
            return fn()
    return run


def reference_style_detection(mov):
    from scipy import ndimage
    for frame in mov:
        dog = ndimage.gaussian_filter(frame, sigma=1.0) - ndimage.gaussian_filter(frame, sigma=2.0)
        tc.peak_local_max(dog, min_distance=3, threshold_abs=0.1 * np.max(dog), exclude_border=False)


def reference_style_fit(patches):
    from scipy.optimize import curve_fit
    P = patches.shape[1]
    x, y = np.meshgrid(np.arange(P), np.arange(P))

    def model(c, amplitude, x0, y0, sigma, offset):
        return (offset + amplitude * np.exp(-((c[0] - x0) ** 2 + (c[1] - y0) ** 2) / (2 * sigma ** 2))).ravel()

    for p in patches:
        try:
            curve_fit(model, (x, y), p.ravel(), p0=(p.max(), P // 2, P // 2, 1.0, p.min()))
        except RuntimeError:
            pass


def bench_linking(mov_gpu, cpu_frames):
    """Linking alone on the detections of a movie: host loop, restatement, device."""
    res = {}
    count, coords, _, _ = ops.dog_peaks(mov_gpu, W1, W2, 0.1, 3, 512, False)
    res["detections_per_frame"] = float(count.float().mean())
    res["gpu_link_frames_s"] = t_events(lambda: ops.link_frames(coords, count, 15.0))
    link = ops.link_frames(coords, count, 15.0)
    res["gpu_chain_tracks_s"] = t_events(lambda: ops.chain_tracks(link, count))

    def device_linking():
        lk = ops.link_frames(coords, count, 15.0)
        ids, lengths, _ = ops.chain_tracks(lk, count)
        T._detections_table(coords, count, ids, lengths, 3)
    res["gpu_linking_s"] = t_events(device_linking)
    for max_gap in (2, ops.LINK_MAX_GAP):
        res[f"gpu_close_gaps_{max_gap}_s"] = t_events(lambda: ops.close_gaps(coords, count, link, max_gap, 15.0))
    res["gap_links_2"] = int((ops.close_gaps(coords, count, link, 2, 15.0)[1] > 0).sum())
    n = count.cpu().numpy()
    host = coords.cpu().numpy().astype(np.int64)
    per_frame = [host[f, :n[f]] for f in range(len(n))]
    res["host_loop_linking_s"] = t_wall(lambda: T._link_tracks(per_frame, 15, 3), reps=2)
    m = min(len(n), cpu_frames)
    res["restatement_linking_s_per_frame"] = t_wall(lambda: T.link_particles_movie(per_frame[:m], None, 15)) / max(m, 1)
    return res


NORM = (20.0, 4.5, 260.0)       # background mean, background sigma, theoretical maximum of the synthetic movies
SEQ_LEN = 5


def bench_diffusion(mov_gpu):
    """The stage after the front end, from the detections table on the device to the model's input and the MSD estimates:
    tracks_table_by_track + the fit (refine_localizations_tensors) + ops.track_msd + track_sequences, against what the same
    took before csrc/diffusion.hip: extract_patches_flat + normalize_images, refine_localizations on the host and a Python
    loop of helpers/msd calls per track.  Events around each, minimum of 5; the second ends on the host."""
    from moleculardiffusion_mivit_amd.helpers import msd as MSD
    from moleculardiffusion_mivit_amd.helpers.generation import normalize_images
    res = {}
    table, _ = T.track_particles_tensors(mov_gpu, return_dog=False)
    fr, y, x, tid, off = T.tracks_table_by_track(table)
    off32 = off.int()
    fit = T.refine_localizations_tensors(T.extract_patches_flat(mov_gpu, fr, y, x, PATCH), y, x)
    pos = torch.stack([fit["y_refined"], fit["x_refined"]], dim=1)
    lengths = (off[1:] - off[:-1]).cpu().numpy()
    res["diffusion_tracks"], res["diffusion_rows"] = int(len(lengths)), int(len(fr))
    res["diffusion_longest_track"] = int(lengths.max()) if len(lengths) else 0
    res["gpu_track_msd_s"] = t_events(lambda: ops.track_msd(pos, off32, 1.0, 0, res["diffusion_longest_track"]))
    res["gpu_track_sequences_s"] = t_events(lambda: T.track_sequences(mov_gpu, fr, y, x, off, SEQ_LEN, PATCH, NORM))
    res["diffusion_sequences"] = int(len(T.plan_sequences(off, SEQ_LEN)[0]))

    def device_stage():
        f, yy, xx, _, o = T.tracks_table_by_track(table)
        ft = T.refine_localizations_tensors(T.extract_patches_flat(mov_gpu, f, yy, xx, PATCH), yy, xx)
        ops.track_msd(torch.stack([ft["y_refined"], ft["x_refined"]], dim=1), o.int(), 1.0, 0)
        T.track_sequences(mov_gpu, f, yy, xx, o, SEQ_LEN, PATCH, NORM)

    def host_shaped_stage():
        keep = table["in_long_track"]
        cols = [table[k][keep] for k in ("frame", "y", "x", "track_id")]
        order = torch.argsort(cols[3], stable=True)
        f, yy, xx, ids = (c[order] for c in cols)
        patches = T.extract_patches_flat(mov_gpu, f, yy, xx, PATCH)
        normed, _ = normalize_images(patches, *NORM)
        ft = T.refine_localizations(patches, yy, xx)
        p = np.stack([ft["y_refined"], ft["x_refined"]], axis=1)
        ids = ids.cpu().numpy()
        cuts = np.flatnonzero(np.diff(ids)) + 1
        seqs = []
        for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(ids)]])):
            msd = MSD.mean_square_displacements(p[None, a:b])
            t = np.arange(b - a) * 1.0
            MSD.estimateDfromMSDs(msd, t)
            MSD.estimateDfromMSDsWeighted(msd, t)
            n = (b - a) // SEQ_LEN
            seqs.append(normed[a:a + n * SEQ_LEN].reshape(n, SEQ_LEN, PATCH, PATCH))
        if seqs:
            torch.cat(seqs)

    res["gpu_diffusion_stage_s"] = t_events(device_stage)
    res["host_shaped_diffusion_stage_s"] = t_events(host_shaped_stage)
    return res


def bench(name, mov_gpu, cpu_frames):
    F, H, W = mov_gpu.shape
    res = {"shape": [F, H, W]}
    res["gpu_detect_s"] = t_events(lambda: ops.dog_peaks(mov_gpu, W1, W2, 0.1, 3, 512, True))
    tracks, det, _ = quiet(lambda: T.track_particles_flat(mov_gpu))()
    res["detections"], res["tracks"] = int(len(det["frame"])), len(tracks)
    rows = np.array([(fr, y, x) for pos in tracks.values() for fr, y, x in pos]).reshape(-1, 3)
    patches = T.extract_patches_flat(mov_gpu, rows[:, 0], rows[:, 1], rows[:, 2], PATCH)
    res["fits"] = int(len(rows))
    res["gpu_fit_s"] = t_events(lambda: ops.refine_gaussian(patches))
    _, _, st = ops.refine_gaussian(patches)
    res["fits_not_converged"] = int((st != 0).sum())

    def whole(linking="host", max_gap=0):
        T.track_particles_flat(mov_gpu, linking=linking, max_gap=max_gap)
        torch.cuda.synchronize()
    res["gpu_track_particles_s"] = t_wall(quiet(whole), reps=5)
    quiet(lambda: whole("device"))()
    res["gpu_track_particles_device_linking_s"] = t_wall(quiet(lambda: whole("device")), reps=5)
    res["gpu_track_particles_device_linking_max_gap_0_s"] = t_wall(quiet(lambda: whole("device", 0)), reps=5)
    quiet(lambda: whole("device", 2))()
    res["gpu_track_particles_device_linking_max_gap_2_s"] = t_wall(quiet(lambda: whole("device", 2)), reps=5)
    res.update(bench_linking(mov_gpu, cpu_frames))
    res.update(bench_diffusion(mov_gpu))
    n = min(F, cpu_frames)
    res["cpu_frames"] = n
    mov = mov_gpu[:n].cpu().numpy()
    res["numpy_detect_s_per_frame"] = t_wall(lambda: T.detect_particles_movie(mov)) / n
    res["reference_style_detect_s_per_frame"] = t_wall(lambda: reference_style_detection(mov)) / n
    m = min(len(rows), 2000)
    pat = patches[:m].cpu().numpy()
    res["cpu_fits"] = m
    res["numpy_fit_s_per_patch"] = t_wall(lambda: T._refine_numpy(pat)) / max(m, 1)
    res["reference_style_fit_s_per_patch"] = t_wall(lambda: reference_style_fit(pat[:500])) / max(min(m, 500), 1)
    if n == F:
        res["numpy_track_particles_s"] = t_wall(quiet(lambda: T.track_particles_flat(mov)))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=20)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"fixture": bench("fixture", torch.from_numpy(tc.movie("main")).cuda(), 30)}
    if not a.small_only:
        out["large"] = bench("large", gpu_movie(1000, 512, 512, 50), a.cpu_frames)
        dense = gpu_movie(1000, 512, 512, 200, seed=1)
        out["dense"] = {"shape": list(dense.shape), **bench_linking(dense, a.cpu_frames)}

        def whole(linking):
            T.track_particles_flat(dense, linking=linking)
            torch.cuda.synchronize()
        quiet(lambda: whole("device"))()
        out["dense"]["gpu_track_particles_s"] = t_wall(quiet(lambda: whole("host")), reps=2)
        out["dense"]["gpu_track_particles_device_linking_s"] = t_wall(quiet(lambda: whole("device")), reps=5)
        print("dense", json.dumps(out["dense"]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
