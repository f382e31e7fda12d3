"""Shared by tests/test_gap_closing.py and tests/test_gap_closing_gpu.py: the scenes of the gap-closing tests.  Every expected
value here is written by hand or derived from how the scene is planted; the restatement (helpers/tracking.py) is held against
them on the CPU, the kernels against the restatement on the GPU.

The hand case (max_gap = 2, max_distance = 15, seven frames, (y, x)):
  P  (10, 10) in frames 0, 1, dark in frame 2, (11, 13) in frames 3 .. 5: a one-frame gap closed in pass 2; the filled row
     lands on (10.5, 11.5), which rounds half to even to (10, 12).
  Q  (40, 40) in frames 0, 1, dark in frame 2, back at (40, 50) in frames 3 .. 5: closed in pass 2 over 10 pixels.
  R  (40, 41) from frame 4: one pixel from Q's end in frame 1, nearer than Q's own return, but pass 3 comes after pass 2 and
     the end is taken: R opens a track.
  U  (100, 105) in frames 0 .. 2;  T (100, 121) in frame 3 only;  S (100, 100) in frame 5.  Pass 2 pairs T with S (nothing else
     is open in frames 3 and 5) and drops the pair at 21 pixels; both stay open, and pass 3 links S to U over 5 pixels.  U to T
     in consecutive frames is 16 pixels: no link.
  V  (150, 20) in frame 0 and again in frame 4: three missed frames, longer than max_gap.
  W  (150, 20) in frame 6, which opens a new movie: the gap to V's row of frame 4 is blocked.
Detections are shuffled within the frames so that no index map is the identity."""
import numpy as np

import linking_common as lc

HAND_MAX_GAP = 2
HAND_MAX_DISTANCE = 15
HAND_FRAMES = [
    np.array([[10, 10], [40, 40], [100, 105], [150, 20]]),          # P Q U V
    np.array([[40, 40], [100, 105], [10, 10]]),                     # Q U P
    np.array([[100, 105]]),                                         # U
    np.array([[100, 121], [11, 13], [40, 50]]),                     # T P Q
    np.array([[11, 13], [40, 41], [40, 50], [150, 20]]),            # P R Q V
    np.array([[100, 100], [40, 41], [40, 50], [11, 13]]),           # S R Q P
    np.array([[150, 20]]),                                          # W
]
HAND_MOVIE_START = np.array([0, 0, 0, 0, 0, 0, 1], np.uint8)
HAND_COUNTS = np.array([4, 3, 1, 3, 4, 4, 1], np.int32)
HAND_LINK = np.array([[-1, -1, -1, -1],
                      [1, 2, 0, -1],
                      [1, -1, -1, -1],
                      [-1, -1, -1, -1],
                      [1, -1, 2, -1],
                      [-1, 1, 2, 0],
                      [-1, -1, -1, -1]], np.int32)
HAND_GAP_PARTNER = np.array([[-1, -1, -1, -1],
                             [-1, -1, -1, -1],
                             [-1, -1, -1, -1],
                             [-1, 2, 0, -1],                        # P and Q of frame 3 <- frame 1
                             [-1, -1, -1, -1],
                             [0, -1, -1, -1],                       # S of frame 5 <- U of frame 2
                             [-1, -1, -1, -1]], np.int32)
HAND_GAP_FRAMES = np.array([[0, 0, 0, 0],
                            [0, 0, 0, 0],
                            [0, 0, 0, 0],
                            [0, 2, 2, 0],
                            [0, 0, 0, 0],
                            [3, 0, 0, 0],
                            [0, 0, 0, 0]], np.int32)
# ids: P 0, Q 1, U (and S) 2, V 3, T 4, R 5, V again 6, W 7
HAND_IDS = np.array([[0, 1, 2, 3],
                     [1, 2, 0, -1],
                     [2, -1, -1, -1],
                     [4, 0, 1, -1],
                     [0, 5, 1, 6],
                     [2, 5, 1, 0],
                     [7, -1, -1, -1]], np.int32)
HAND_LENGTHS = [5, 5, 4, 1, 1, 2, 1, 1]                              # detections per track
# (frame, y, x, id) of the filled rows: 10.5 -> 10 and 11.5 -> 12 (half to even); 105 - 5 / 3 = 103.33, 105 - 10 / 3 = 101.67
HAND_FILLED = [(2, 10, 12, 0), (2, 40, 45, 1), (3, 100, 103, 2), (4, 100, 102, 2)]


def hand_padded():
    padded = np.zeros((len(HAND_FRAMES), 4, 2), np.int32)
    for f, c in enumerate(HAND_FRAMES):
        padded[f, :len(c)] = c
    return padded


WALK_SPEC = (131, 60, 50, 3.0, 0.05, 3)           # linking_common.walk_sequence(seed, 60, 50, 3.0, 0.05, 3)
WALK_MAX_GAPS = (1, 3, 8)


def walk_padded(cap=None):
    """The drop-out sequence of the structure test, padded -> (coords [60, cap, 2] int32, counts [60] int32)."""
    frames = lc.walk_sequence(*WALK_SPEC)
    counts = np.array([len(c) for c in frames], np.int32)
    cap = cap or int(counts.max())
    padded = np.zeros((len(frames), cap, 2), np.int32)
    for f, c in enumerate(frames):
        padded[f, :len(c)] = c
    return padded, counts


# ---- planted dark runs on a lattice ----------------------------------------------------------------------------------
LATTICE_STEP, LATTICE_SIDE, LATTICE_FRAMES, LATTICE_WANDER = 40, 3, 62, 5


def lattice_scene():
    """Nine particles around the points of a 40-pixel lattice, steps of at most one pixel per axis and frame, never more than
    5 pixels from their lattice point.  Particle i is dark for 1 + i % 3 frames from frame 4 + 6 i on: the runs lie strictly
    inside the sequence and at least three frames apart, so no frame has more than one open end or one open start and the
    only end / start pairs at most four frames apart belong to one particle (its return lies at most 4 * sqrt(2) = 5.7 pixels
    from where it left).  -> (frames: list of int64 [n, 2], run lengths [9], owner: list of particle indices per frame)."""
    rng = np.random.default_rng(7)
    n = LATTICE_SIDE * LATTICE_SIDE
    home = np.array([[30 + LATTICE_STEP * (i // LATTICE_SIDE), 30 + LATTICE_STEP * (i % LATTICE_SIDE)] for i in range(n)])
    off = np.zeros((n, 2), np.int64)
    runs = np.array([1 + i % 3 for i in range(n)])
    first_dark = np.array([4 + 6 * i for i in range(n)])
    frames, owner = [], []
    for f in range(LATTICE_FRAMES):
        off = np.clip(off + rng.integers(-1, 2, (n, 2)), -LATTICE_WANDER, LATTICE_WANDER)
        seen = np.flatnonzero(~((first_dark <= f) & (f < first_dark + runs)))
        seen = seen[rng.permutation(len(seen))]
        frames.append((home + off)[seen])
        owner.append(seen)
    assert first_dark[-1] + runs[-1] < LATTICE_FRAMES - 1
    return frames, runs, owner


# ---- a simulated movie with blinking particles -----------------------------------------------------------------------
SIM_FRAMES, SIM_SIDE, SIM_PARTICLES = 40, 64, 3
SIM_PROPS = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}          # noise-free
# (particle, first dark frame, run length)
SIM_DARK = [(0, 8, 1), (0, 20, 2), (1, 14, 2), (2, 27, 1)]
SIM_D, SIM_NPOS, SIM_SEED = 0.05, 3, 9      # seed 9: the particles never come within 19 pixels of each other


def sim_blink_mask():
    mask = np.zeros((SIM_PARTICLES, SIM_FRAMES), bool)
    for p, f, n in SIM_DARK:
        mask[p, f:f + n] = True
    return mask


def sim_movie():
    """-> (movie [40, 64, 64] float32 CPU tensor, truth): three slow particles, noise-free, dark as SIM_DARK plants it."""
    import torch
    from moleculardiffusion_mivit_amd.helpers import generation as gen
    return gen.simulate_movie(SIM_PARTICLES, SIM_FRAMES, SIM_SIDE, SIM_SIDE, SIM_D, SIM_NPOS, image_props=SIM_PROPS,
                              generator=torch.Generator().manual_seed(SIM_SEED), blink=torch.from_numpy(sim_blink_mask()))
