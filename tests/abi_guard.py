"""Guarded, poisoned buffers for tests that call the C-ABI directly (tests/test_analysis_abi_gpu.py,
tests/test_simulation_abi_gpu.py, through the harness of tests/abi_call.py): tests/gpu_buffers.py for any element type.
Plain torch + ctypes; works on the CPU too, which is how tests/test_abi_guard.py tests the harness itself.

A Buf is ONE allocation laid out as [guard | body | guard].  The body has exactly the size the header states for the argument,
so a kernel that writes one element past its output, or uses more workspace than it reports, changes a guard; and whatever the
kernel has not written still holds the fill pattern, so an entry the header calls "not written" can be told from one that is,
and a value the kernel had no business reading shows up in its results.

Patterns: POISON is all-ones bits (a NaN in fp32 / fp64, -1 in int32, 0xFF in bytes) and fills the guards always.  GARBAGE
(0x3A in every byte: 976 894 522 as int32, 4.6e-4 as fp32) is for integer buffers in which -1 is a legal value (links, ids,
states): a stray read of it changes a distance or an index, an unwritten output cannot be mistaken for a written -1.

Hostile indices are planted through `bounded` alone, which keeps every out-of-range value within g rows of the valid range
with g * row bytes <= guard_bytes: were a clamp missing, the stray access would still land inside the test's own allocation."""
import numpy as np
import torch

POISON, GARBAGE, ZERO = 0xFF, 0x3A, 0x00
FILLS = {"poison": POISON, "garbage": GARBAGE, "zero": ZERO}
GUARD_BYTES = 4096
ALIGN = 256


def _device():
    return "cuda" if torch.cuda.is_available() else "cpu"


def _as_tensor(values, dtype):
    if not torch.is_tensor(values):
        values = torch.from_numpy(np.array(values, order="C"))            # a copy: read-only arrays are welcome
    return values.detach().cpu().to(dtype).contiguous()


class Buf:
    """values (array / tensor, converted to dtype) or a shape; fill names the pattern of a body given by shape.  misalign=k
    moves the body k elements off the 256-byte boundary (natural alignment only, as a contiguous slice hands out)."""

    def __init__(self, values_or_shape, dtype, guard_bytes=GUARD_BYTES, misalign=0, fill="poison", device=None):
        self.dtype, self.guard_bytes = dtype, int(guard_bytes)
        self.esize = torch.empty(0, dtype=dtype).element_size()
        if isinstance(values_or_shape, (tuple, list, int)):
            self.shape = (values_or_shape,) if isinstance(values_or_shape, int) else tuple(int(s) for s in values_or_shape)
            init = None
        else:
            init = _as_tensor(values_or_shape, dtype)
            self.shape = tuple(init.shape)
        self.numel = int(np.prod(self.shape, dtype=np.int64)) if len(self.shape) else 1
        self.nbytes = self.numel * self.esize
        assert self.guard_bytes >= self.esize and misalign >= 0
        device = device or _device()
        # room to put the body on a 256-byte boundary whatever the allocator returns, then `misalign` elements further
        raw = torch.full((self.guard_bytes + 2 * ALIGN + misalign * self.esize + self.nbytes + self.guard_bytes,), POISON,
                         dtype=torch.uint8, device=device)
        base = raw.data_ptr()
        self.off = (-(base + self.guard_bytes)) % ALIGN + self.guard_bytes + misalign * self.esize
        self.raw = raw[:self.off + self.nbytes + self.guard_bytes]
        self.ptr = base + self.off
        assert (self.ptr - misalign * self.esize) % ALIGN == 0 and self.ptr % self.esize == 0
        if init is not None:
            self._put(init.reshape(-1).view(torch.uint8) if self.numel else torch.empty(0, dtype=torch.uint8))
        elif FILLS[fill] != POISON:
            self.raw[self.off:self.off + self.nbytes] = FILLS[fill]
        self._initial = self.body_bytes()

    def _put(self, b):
        self.raw[self.off:self.off + self.nbytes] = b.to(self.raw.device)

    def write(self, values):
        """new body contents (the reference for `untouched` moves with them)"""
        t = _as_tensor(values, self.dtype)
        assert tuple(t.shape) == self.shape, (tuple(t.shape), self.shape)
        self._put(t.reshape(-1).view(torch.uint8))
        self._initial = self.body_bytes()

    def refill(self, byte):
        """every body byte = byte (a workspace before a call)"""
        self.raw[self.off:self.off + self.nbytes] = int(byte)
        self._initial = self.body_bytes()

    def body_bytes(self):
        return self.raw[self.off:self.off + self.nbytes].cpu().clone()

    def body(self):
        """the body as a CPU tensor of the buffer's dtype and shape (a copy)"""
        return self.body_bytes().view(self.dtype).reshape(self.shape)

    def numpy(self):
        return self.body().numpy()

    def guards_intact(self):
        r = self.raw.cpu()
        return bool((r[:self.off] == POISON).all()) and bool((r[self.off + self.nbytes:] == POISON).all())

    def _elementwise(self, same_bytes):
        return same_bytes.reshape(self.numel, self.esize).all(dim=1).reshape(self.shape)

    def unchanged(self):
        """bool [shape]: the elements that are bitwise what the body held before the call"""
        return self._elementwise(self.body_bytes() == self._initial)

    def untouched(self, mask=None):
        """every element of mask (all of the body if None) is bitwise what it was before the call"""
        same = self.unchanged()
        if mask is None:
            return bool(same.all())
        mask = torch.as_tensor(np.asarray(mask), dtype=torch.bool).reshape(self.shape)
        return bool(same[mask].all())

    def poisoned(self):
        """bool [shape]: the elements whose every byte is POISON"""
        return self._elementwise(self.body_bytes() == POISON)


def is_poison(t):
    """bool mask of the elements of a CPU tensor / array that are the all-ones pattern"""
    t = torch.as_tensor(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.contiguous()
    es = t.element_size()
    return (t.reshape(-1).view(torch.uint8).reshape(-1, es) == POISON).all(dim=1).reshape(t.shape)


def rows_within_guard(row_bytes, guard_bytes=GUARD_BYTES, most=64):
    """g: how many rows of row_bytes a hostile index may lie outside its valid range"""
    assert row_bytes >= 1
    return min(most, guard_bytes // row_bytes)


def bounded(values, lo, hi, row_bytes, guard_bytes=GUARD_BYTES):
    """The hostile indices of a test: int32 array of `values`, every one of which lies in [lo - g, hi + g] where [lo, hi] is
    the valid range of the index and g = rows_within_guard(row_bytes): an unclamped access through it stays inside the guards
    of a Buf of such rows.  row_bytes: the LARGEST row any buffer indexed by these values has.  Asserts."""
    v = np.asarray(values, dtype=np.int64)
    g = rows_within_guard(row_bytes, guard_bytes)
    assert g >= 1, f"rows of {row_bytes} bytes do not fit a guard of {guard_bytes} bytes"
    assert v.size == 0 or (v.min() >= lo - g and v.max() <= hi + g), \
        f"hostile index outside [{lo} - {g}, {hi} + {g}]: {int(v.min())} .. {int(v.max())} (rows of {row_bytes} bytes)"
    return v.astype(np.int32)


def same_bits(a, b):
    """bitwise equality of two arrays / CPU tensors of one dtype and shape (NaN payloads and the sign of zero included)"""
    a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
