"""Shared by tests/test_linking.py, tests/test_linking_gpu.py, tests/golden/make_link_golden.py and scripts/bench_tracking.py:
the seeded detection sequences of the linking fixture, its file layout, and the bars with their origin.

The fixture (tests/golden/tracking_link/link.npz) holds, per case, the detections of a short sequence of frames and, for every
pair of consecutive frames, the links the reference's own link_particles returned (max_distance filter applied) plus a flag:
true when that link set came out the same under ORDER_PERMUTATIONS random permutations of rows and columns.  Where it did
not, the pair has several optimal assignments (ties of integer geometry) and scipy's choice depends on the order of its
rows; only the total cost is then comparable.

The bars
  Links.  Integers: equality, on every flagged pair.
  Total cost.  Two optimal assignments of one matrix differ only by the rounding of their sums: COST_RTOL = 1e-9 relative
  (1e-12 was the largest difference seen on 1 000-frame sequences; the bar leaves three orders for larger frames).
  False flags.  In the 12- and 50-particle sequences at most MAX_FALSE_FRACTION = 2 % of the pairs may be order dependent
  (measured on 1 000-frame sequences of the same kind: 0 %, 0.7 %, 0.5 %); asserted when the fixture is written and read."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_link")
GOLDEN = os.path.join(GOLDEN_DIR, "link.npz")

MAX_DISTANCE = 15
ORDER_PERMUTATIONS = 8
COST_RTOL = 1e-9
MAX_FALSE_FRACTION = 0.02
FIELD = 512

# name -> (seed, frames, particles, step in px, drop-out probability, spurious points per frame)
SEQUENCES = {
    "p12": (101, 300, 12, 1.0, 0.0, 0),
    "p50_step1": (102, 300, 50, 1.0, 0.0, 0),
    "p50_step3": (113, 300, 50, 3.0, 0.05, 3),
}
BOUNDED = tuple(SEQUENCES)            # the cases the false-flag condition applies to


def walk_sequence(seed, frames, particles, step, dropout, spurious, field=FIELD):
    """Random walks rounded to pixels, with drop-outs and spurious points, shuffled within each frame -> list of int64 [n, 2]."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, field, (1, particles, 2)) + np.cumsum(rng.normal(0.0, step, (frames, particles, 2)), axis=0)
    out = []
    for f in range(frames):
        pts = np.rint(pos[f][rng.random(particles) >= dropout]).astype(np.int64)
        if spurious:
            pts = np.concatenate([pts, rng.integers(0, field, (spurious, 2))])
        out.append(pts[rng.permutation(len(pts))])
    return out


def special_cases():
    """Rectangular and degenerate pairs and the 512 x 512 pair, each a sequence of two frames."""
    rng = np.random.default_rng(104)
    e = np.zeros((0, 2), np.int64)
    a = rng.integers(0, 120, (17, 2))
    near = a + rng.integers(-2, 3, a.shape)
    big0 = rng.integers(0, 2048, (512, 2))
    return {
        "more_before": [rng.integers(0, 80, (14, 2)), rng.integers(0, 80, (9, 2))],
        "more_after": [rng.integers(0, 80, (6, 2)), rng.integers(0, 80, (15, 2))],
        "empty_before": [e, rng.integers(0, 80, (5, 2))],
        "empty_after": [rng.integers(0, 80, (5, 2)), e],
        "both_empty": [e, e],
        "single_point": [np.array([[10, 12]]), np.array([[13, 16]])],
        "single_to_many": [np.array([[40, 40]]), rng.integers(30, 50, (6, 2))],
        "identical_frames": [a, a.copy()],
        "small_moves": [a, near[rng.permutation(len(a))]],
        "all_beyond_max_distance": [rng.integers(0, 50, (8, 2)), rng.integers(300, 350, (8, 2))],
        "full_512": [big0, (big0 + np.rint(rng.normal(0, 4.0, big0.shape)).astype(np.int64))[rng.permutation(512)]],
    }


def cases():
    out = {name: walk_sequence(*spec) for name, spec in SEQUENCES.items()}
    out.update(special_cases())
    return out


def load():
    """-> {case: (frames: list of int64 [n, 2], links: list per pair of sets {(i0, i1)}, flags: bool per pair)}."""
    z = np.load(GOLDEN)
    out = {}
    for name in [str(n) for n in z["cases"]]:
        counts, flat = z[f"{name}_counts"], z[f"{name}_coords"].astype(np.int64)
        ends = np.cumsum(counts)
        frames = [flat[e - c:e] for c, e in zip(counts, ends)]
        rows = z[f"{name}_links"]
        links = [set() for _ in range(len(frames) - 1)]
        for p, i0, i1 in rows:
            links[p].add((int(i0), int(i1)))
        out[name] = (frames, links, z[f"{name}_order_independent"])
    return out


def link_set(link_row, n1):
    return {(int(link_row[j]), j) for j in range(n1) if link_row[j] >= 0}
