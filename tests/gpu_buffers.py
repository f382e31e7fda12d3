"""Device buffers of the operator-level GPU suites (tests/test_operators_gpu.py, tests/test_streaming_ops_gpu.py): strided inputs
with NaN padding, outputs with a sentinel everywhere outside the result."""
import torch

from operators_common import DT, ESIZE

SENT = {2: 0x7E57, 4: 0x7FC0BEEF}
ITYPE = {2: torch.int16, 4: torch.int32}


def inp(vals, dt, ld=None, off=0, rows=None, total=None):
    """fp32 values [R, C] -> (device buffer, pointer): rows `rows` of `total` rows of stride ld, `off` elements into the
    allocation, NaN everywhere else"""
    R, C = vals.shape
    ld = ld or C
    total = total or R
    flat = torch.full((off + total * ld,), float("nan"), dtype=DT[dt])
    flat[off:].view(total, ld)[rows if rows is not None else slice(None), :C] = vals.to(DT[dt])
    g = flat.cuda()
    return g, g.data_ptr() + off * ESIZE[dt]


class Out:
    """output of `total` rows of stride ld, `off` elements into the allocation, one guard row before and after; everything
    but columns < ncols of the rows `rows` must keep the sentinel.  The guard in front is padded to a multiple of 8 elements
    (16 or 32 bytes), so the alignment of the pointer the kernel sees is that of `off` alone, as the restatements assume"""

    def __init__(self, dt, total, ncols, ld, off=0, rows=None, init=None):
        self.dt, self.total, self.ncols, self.ld, self.off = dt, total, ncols, ld, off
        self.front = (ld + 7) // 8 * 8
        self.rows = torch.arange(total) if rows is None else rows
        es = ESIZE[dt]
        flat = torch.full((off + self.front + (total + 1) * ld,), SENT[es], dtype=ITYPE[es])
        if init is not None:
            self._body(flat)[self.rows, :ncols] = init.to(DT[dt]).view(ITYPE[es])
        self.raw = flat.cuda()
        self.ptr = self.raw.data_ptr() + (off + self.front) * es
        assert self.raw.data_ptr() % 256 == 0

    def _body(self, flat):
        a = self.off + self.front
        return flat[a:a + self.ld * self.total].view(self.total, self.ld)

    def read(self):
        flat = self.raw.cpu()
        keep = torch.ones(flat.numel(), dtype=torch.bool)
        self._body(keep)[self.rows, :self.ncols] = False
        assert bool((flat[keep] == SENT[ESIZE[self.dt]]).all()), "the kernel wrote outside its output"
        return self._body(flat)[self.rows, :self.ncols].contiguous().view(DT[self.dt])
