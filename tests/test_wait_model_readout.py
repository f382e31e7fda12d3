"""Host replay (tests/test_wait_model.py) of the tile wait of attn_out_bwd_kernel<ROWS = true> (csrc/fused_bwd.hip).

Requests AND the dctx stores can be absent for a wave, so no count describes the queue: the kernel waits vmcnt(0), restated
here so that a change back to a counted wait is checked against the case that breaks it."""
import itertools

import pytest

from test_wait_model import Wave


def attn_out_rows(tiles, wait):
    """tiles: per tile (pieces requested, dz1 stores before the prefetch, dctx stores after it) of one wave"""
    w = Wave()
    w.issue(("P", 0), tiles[0][0])
    for t, (p, early, late) in enumerate(tiles):
        w.wait(0 if t == 0 else wait)
        if p:
            w.need(("P", t))
        w.issue(("dz", t), early)
        w.issue(("P", t + 1), tiles[min(t + 1, len(tiles) - 1)][0])
        w.issue(("st", t), late)


def test_attn_out_bwd_rows_wait_is_zero():
    shapes = [(0, 0, 0), (4, 1, 4), (8, 2, 4), (4, 1, 0)]
    for tiles in itertools.product(shapes, repeat=3):
        attn_out_rows(tiles, 0)
    # the full kernel's count, four row stores, is wrong as soon as a wave skips them: a tile without stores in front of a tile
    # with requests
    with pytest.raises(AssertionError):
        attn_out_rows([(4, 1, 0), (4, 1, 0), (4, 1, 0)], 4)
