"""Time of the filament-mapping kernel (helpers/geometry.map_displacements -> ops.map_displacements -> csrc/confine.hip) and of
its numpy restatement on the same input, in both boundary modes.  Events on the stream after a warm-up, minimum of 5; the
restatement once, by the wall clock.  kernel_ms is the launch alone: the C entry on pre-validated device tensors into
outputs allocated once (ops._map_displacements_checked); ops_call_ms is ops.map_displacements, which also reads vert_offsets
and the range of geom_of back to validate them and allocates the outputs; call_ms is the front end,
geometry.map_displacements, from device displacements and starts and a host packing uploaded once.  Shapes, all on the
reference notebook's ten-edge serpentine (total length 1550) with steps of sigma 25: N = 352 / T = 3000, N = 4096 / T = 2048 and N = 20 / T = 10 000 (the 1000-frame, 10 sub-position movie of
scripts/bench_tracking.py).  Every GPU step is followed by a synchronisation and an error check of its own; the first error ends
the script with a non-zero status, nothing further is started.  The kernel's result is compared bitwise with the restatement's.

    python scripts/bench_geometry.py [--small-only] [--json OUT]
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
from moleculardiffusion_mivit_amd.helpers import geometry as geo


def checked(what, fn):
    """one GPU step under its own check: run, wait for it, and leave on the first error"""
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception as exc:                                 # noqa: BLE001  (whatever went wrong, nothing more is started)
        print(f"bench_geometry: {what} failed: {exc}", file=sys.stderr, flush=True)
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


def bench_shape(N, T, g):
    rng = np.random.default_rng(0)
    disp = rng.standard_normal((N, T)) * 25.0
    s0 = rng.uniform(0, g.total_length, N)
    packed = geo.pack_geometries(g)
    dev = checked("upload", lambda: {k: torch.from_numpy(v).cuda() for k, v in packed.items()})
    dd, sd = checked("upload", lambda: (torch.from_numpy(disp).cuda(), torch.from_numpy(s0).cuda()))
    gof = checked("upload", lambda: torch.zeros(N, dtype=torch.int32, device="cuda"))
    row = {"N": N, "T": T, "edges": len(g.edges), "lds_bytes_per_workgroup": (3 * ops.GEOM_MAX_EDGES + 2 + ops.GEOM_CHUNK_T) * 8}
    for mode in geo.BOUNDARIES:
        args = (dd, sd, gof, dev["verts"], dev["lengths"], dev["vert_offsets"], dev["totals"])
        out = checked("allocate", lambda: (torch.empty(N, T, 2, dtype=torch.float64, device="cuda"),
                                           torch.empty(N, T, dtype=torch.float64, device="cuda"),
                                           torch.empty(N, T, dtype=torch.int32, device="cuda")))
        code = geo.BOUNDARIES.index(mode)
        run = lambda: ops._map_displacements_checked(*args, code, out=out)  # noqa: E731
        t_kernel = checked(f"kernel {mode} N {N} T {T}", lambda: t_events(run))
        t_ops = checked(f"ops call {mode} N {N} T {T}", lambda: t_events(lambda: ops.map_displacements(*args, mode)))
        t_call = checked(f"call {mode} N {N} T {T}", lambda: t_events(lambda: geo.map_displacements(dd, sd, packed, None, mode, True)))
        got = checked(f"download {mode}", lambda: [o.cpu().numpy() for o in run()])
        t0 = time.perf_counter()
        want = geo.map_displacements(disp, s0, packed, None, mode, True)
        t_cpu = time.perf_counter() - t0
        equal = all(np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
                    for a, b in zip(got, want))
        # bytes the kernel has to move: disp in, pos, arc and edge out
        row[mode] = {"kernel_ms": t_kernel * 1e3, "ops_call_ms": t_ops * 1e3, "call_ms": t_call * 1e3, "ns_per_step_of_one_particle": t_kernel * 1e9 / T,
                     "gb_per_s": N * T * (8 + 16 + 8 + 4) / t_kernel * 1e-9, "cpu_restatement_ms": t_cpu * 1e3,
                     "bitwise_equal_to_restatement": bool(equal)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry.py needs a GPU")
    g = geo.cristae_geometry(2, 100, (200, 250), 30, lead=100, entry=300, tail=90)      # the notebook's ten-edge serpentine
    assert len(g.edges) == 10 and g.total_length == 1550.0
    shapes = [(352, 3000)] if args.small_only else [(352, 3000), (4096, 2048), (20, 10000)]
    out = []
    for N, T in shapes:
        out.append(bench_shape(N, T, g))
        print(json.dumps(out[-1]), flush=True)
        if not all(out[-1][m]["bitwise_equal_to_restatement"] for m in geo.BOUNDARIES):
            print("bench_geometry: the kernel and the restatement differ", file=sys.stderr, flush=True)
            sys.exit(1)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
