"""The harness around one call of a C-ABI entry inside the guarded buffers of tests/abi_guard.py, shared by
tests/test_analysis_abi_gpu.py and tests/test_simulation_abi_gpu.py: the Bufs of a call and the checks every call gets (Call),
what an output must hold afterwards (expect, check_all), two calls against each other (same_results, bits_equal), and the
host's side of the header's sentence about CSR offsets (sanitise_csr).  Buf works on the CPU, so tests/test_abi_guard.py shows
on the CPU that expect and bits_equal can fail.

Bitwise comparisons treat every NaN as one value (the sign of a computed NaN is the hardware's) and tell -0 from +0."""
import ctypes

import numpy as np
import pytest
import torch

import abi_guard as G
from abi_guard import Buf
from moleculardiffusion_mivit_amd import _native as N

F64, F32, I32, U8 = torch.float64, torch.float32, torch.int32, torch.uint8


class Call:
    """The Bufs of one call of an entry: inputs (must come back bitwise unchanged), outputs, one workspace."""

    def __init__(self, entry, mis=0):
        self.entry, self.mis = entry, mis
        self.ins, self.outs, self.ws = {}, {}, None

    def inp(self, name, values, dtype):
        self.ins[name] = Buf(values, dtype, misalign=self.mis)
        return self.ins[name]

    def out(self, name, shape, dtype, fill=None):
        fill = fill or ("garbage" if dtype == I32 else "poison")
        self.outs[name] = Buf(shape, dtype, misalign=self.mis, fill=fill)
        return self.outs[name]

    def work(self, nbytes, dtype=U8, fill=G.POISON):
        """exactly nbytes bytes, 256-byte aligned as hipMalloc gives it, whatever self.mis is"""
        self.ws = Buf(int(nbytes) // torch.empty(0, dtype=dtype).element_size(), dtype)
        assert self.ws.nbytes == int(nbytes) and self.ws.ptr % 256 == 0
        if torch.is_tensor(fill):                                         # the leftovers of another problem
            self.ws.write(fill)
        else:
            self.ws.refill(fill)
        return self.ws

    def run(self, *args):
        raw = [a.ptr if isinstance(a, Buf) else a for a in args]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        try:
            N.check(getattr(N.lib, self.entry)(*raw, stream), self.entry)
            torch.cuda.synchronize()
        except Exception as e:                                            # a faulted device fails every later call: stop here
            if "hip" in str(e).lower():
                pytest.exit(f"{self.entry}: {e}", returncode=3)
            raise
        for kind, bufs in (("input", self.ins), ("output", self.outs), ("workspace", {"ws": self.ws} if self.ws else {})):
            for name, b in bufs.items():
                assert b.guards_intact(), f"{self.entry}: a guard of the {kind} {name} changed"
        for name, b in self.ins.items():
            assert b.untouched(), f"{self.entry}: the input {name} was written"
        return self


def _nan_mask(a):
    return np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)


def bits_equal(got, want):
    """bitwise, every NaN one value"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    ng, nw = _nan_mask(got), _nan_mask(want)
    return bool(np.array_equal(ng, nw)) and G.same_bits(got[~ng], want[~nw])


def expect(call, name, want, written=None, close=None):
    """The output `name` of a finished call: where `written` (everywhere if None) it holds want (bitwise, or under close) and
    nothing of the fill pattern is left; elsewhere it is bitwise what it was before the call."""
    buf = call.outs[name]
    got = buf.numpy()
    want = np.asarray(want).astype(got.dtype).reshape(got.shape)
    w = np.ones(got.shape, bool) if written is None else np.broadcast_to(np.asarray(written, bool), got.shape)
    same = buf.unchanged().numpy()
    what = f"{call.entry}: {name}"
    assert same[~w].all(), f"{what}: {int((~same[~w]).sum())} entries written that the header says are not written"
    assert not same[w].any(), f"{what}: {int(same[w].sum())} entries the header says are written still hold the fill pattern"
    assert not G.is_poison(got[w]).any() or got.dtype == np.int32, f"{what}: poison in the output"
    if close is None:
        bad = ~((got == want) | (_nan_mask(got) & _nan_mask(want))) & w
        assert bits_equal(got[w], want[w]), f"{what}: {int(bad.sum())} entries differ, first at {np.argwhere(bad)[:3].tolist()}"
    else:
        close(got[w], want[w], what)


def same_results(a, b, names=None):
    """two finished calls wrote bitwise the same outputs"""
    for k in names or a.outs:
        assert bits_equal(a.outs[k].numpy(), b.outs[k].numpy()), f"{a.entry}: {k} differs between the two runs"


def sanitise_csr(raw, n):
    """offsets as the header clamps them -> [(a, b)] per track: a into [0, n], b into [a, n]"""
    out = []
    for k in range(len(raw) - 1):
        a = min(max(int(raw[k]), 0), n)
        b = int(raw[k + 1])
        b = a if b < a else min(b, n)
        out.append((a, b))
    return out


def check_all(call, want, written=None, close=None):
    for name, w in want.items():
        expect(call, name, w, (written or {}).get(name), (close or {}).get(name))


POISON64 = np.frombuffer(b"\xff" * 8, np.float64)[0]
