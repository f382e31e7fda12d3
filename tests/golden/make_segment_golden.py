"""Writes tests/golden/segment/simulate_movie_before_states.npz: one small simulate_movie call on the CPU, recorded on the commit
BEFORE simulate_movie gained the argument `states`, which tests/test_segment.py requires the call without `states` to reproduce bit
for bit.  Run from the repository root of that commit:  python tests/golden/make_segment_golden.py OUT.npz"""
import sys

import numpy as np
import torch

from moleculardiffusion_mivit_amd.helpers import generation as gen

PROPS = {"particle_intensity": [500, 20], "background_intensity": [100, 10], "poisson_noise": 100}

if __name__ == "__main__":
    g = torch.Generator().manual_seed(123)
    vid, truth = gen.simulate_movie(3, 6, 24, 24, (0.5, 0.1), 4, PROPS, generator=g, lifetimes=[[0, 5], [1, 4], [2, 5]])
    np.savez_compressed(sys.argv[1], movie=vid.numpy(), **{k: truth[k].numpy() for k in ("frame", "y", "x", "particle_id",
                                                                                          "offsets", "D", "pos", "amp")})
