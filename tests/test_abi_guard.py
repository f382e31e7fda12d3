"""The guarded-buffer harness (tests/abi_guard.py) can fail: planted writes into either guard and into an untouched region,
a planted read-through and a hostile index beyond the guard are all detected, and a clean run is accepted; so can the checks
of tests/abi_call.py on a finished call (expect, bits_equal).  CPU only: the "kernel" is a few lines of torch on the raw
allocation."""
import numpy as np
import pytest
import torch

import abi_call as A
import abi_guard as G
from abi_guard import Buf

DTYPES = [torch.float64, torch.float32, torch.int32, torch.uint8]


def _body_view(buf):
    """the body of a CPU Buf as a writable flat view of its dtype: what a kernel holding buf.ptr sees"""
    return buf.raw[buf.off:buf.off + buf.nbytes].view(buf.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("misalign", [0, 1, 3])
def test_layout(dtype, misalign):
    b = Buf((5, 3), dtype, misalign=misalign, device="cpu")
    assert b.nbytes == 15 * b.esize and b.body().shape == (5, 3)
    assert (b.ptr - misalign * b.esize) % 256 == 0 and b.ptr == b.raw.data_ptr() + b.off
    assert b.off >= b.guard_bytes and b.raw.numel() == b.off + b.nbytes + b.guard_bytes
    assert b.guards_intact() and b.untouched() and bool(b.poisoned().all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(b.body()).all())
    elif dtype == torch.int32:
        assert bool((b.body() == -1).all())
    else:
        assert bool((b.body() == 0xFF).all())


def test_fills_and_values():
    g = Buf(4, torch.int32, fill="garbage", device="cpu")
    assert g.body().tolist() == [0x3A3A3A3A] * 4 and not bool(g.poisoned().any())
    z = Buf(4, torch.float64, fill="zero", device="cpu")
    assert z.body().tolist() == [0.0] * 4
    v = Buf(np.arange(6, dtype=np.float64).reshape(3, 2), torch.float32, device="cpu")
    assert v.dtype == torch.float32 and v.body().tolist() == [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]] and v.guards_intact()
    e = Buf((0, 2), torch.float64, device="cpu")
    assert e.nbytes == 0 and e.guards_intact() and e.untouched()


def test_clean_run_is_accepted():
    x = Buf(np.arange(8.0), torch.float64, device="cpu")
    y = Buf(8, torch.float64, device="cpu")
    _body_view(y)[:] = 2.0 * _body_view(x)
    assert x.guards_intact() and y.guards_intact() and x.untouched()
    assert not bool(y.poisoned().any()) and G.same_bits(y.body(), torch.arange(8.0, dtype=torch.float64) * 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["front", "back"])
def test_one_element_in_a_guard_is_detected(dtype, side):
    b = Buf(7, dtype, misalign=1, device="cpu")
    at = b.off - b.esize if side == "front" else b.off + b.nbytes          # the element just before / just after the body
    b.raw[at:at + b.esize].view(dtype)[0] = 1
    assert not b.guards_intact()
    assert b.untouched()                                                    # the body itself is as it was


def test_far_end_of_a_guard_is_detected():
    b = Buf(7, torch.float64, device="cpu")
    b.raw[b.raw.numel() - 1] = 0
    assert not b.guards_intact()
    b = Buf(7, torch.float64, device="cpu")
    b.raw[0] = 0
    assert not b.guards_intact()


@pytest.mark.parametrize("fill", ["poison", "garbage"])
def test_write_into_untouched_region_is_detected(fill):
    out = Buf((4, 3), torch.int32, fill=fill, device="cpu")
    count = [2, 0, 3, 1]                                                    # "entries beyond count[f] are not written"
    beyond = np.arange(3)[None, :] >= np.asarray(count)[:, None]
    v = _body_view(out).view(4, 3)
    for f, c in enumerate(count):
        v[f, :c] = 7
    assert out.untouched(beyond) and not out.untouched() and out.guards_intact()
    assert out.unchanged().numpy().tolist() == beyond.tolist()
    v[1, 0] = 7                                                             # one slot past count[1] = 0
    assert not out.untouched(beyond)


def test_rewriting_the_fill_value_counts_as_untouched_only_bitwise():
    out = Buf(3, torch.float32, device="cpu")
    _body_view(out)[1] = float("nan")                                       # a NaN, but not the poison's bits
    assert not out.untouched() and out.poisoned().tolist() == [True, False, True]


def test_read_through_is_detected():
    x = Buf((3, 2), torch.float64, device="cpu")                            # rows 2.. are "not read": poison
    x.write(np.array([[1.0, 2.0], [3.0, 4.0], [np.nan, np.nan]]))
    xp = Buf((3, 2), torch.float64, device="cpu")
    _body_view(xp)[:4] = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    good, bad = Buf(1, torch.float64, device="cpu"), Buf(1, torch.float64, device="cpu")
    _body_view(good)[0] = _body_view(xp)[:4].sum()
    _body_view(bad)[0] = _body_view(xp)[:6].sum()                           # reads the poisoned row
    assert not bool(good.poisoned().any()) and not bool(G.is_poison(good.body()).any())
    assert G.same_bits(good.body(), torch.tensor([10.0], dtype=torch.float64))
    assert not G.same_bits(bad.body(), good.body()) and bool(torch.isnan(bad.body()).all())
    idx = Buf(4, torch.int32, fill="garbage", device="cpu")                 # integer inputs: the garbage changes an index
    assert int(idx.body()[3]) == 0x3A3A3A3A != -1
    assert bool(G.is_poison(np.array([-1, 0, 5], np.int32))[0]) and not bool(G.is_poison(np.array([0x3A3A3A3A], np.int32)).any())


def test_same_bits_tells_zero_signs_and_nan_payloads():
    assert not G.same_bits(np.array([0.0]), np.array([-0.0]))
    assert G.same_bits(np.array([np.nan]), np.array([np.nan]))
    assert not G.same_bits(np.array([np.nan]), Buf(1, torch.float64, device="cpu").numpy())
    assert not G.same_bits(np.zeros(2, np.int32), np.zeros(2, np.int64))


def test_bounded_hostile_indices():
    # g = 64 rows of pos [N, 2] fp64 (16 B) is 1 KiB of a 4 KiB guard
    assert G.rows_within_guard(16) == 64 and G.rows_within_guard(128) == 32 and G.rows_within_guard(8192) == 0
    v = G.bounded([-64, 0, 10, 74], 0, 10, 16)
    assert v.dtype == np.int32 and v.tolist() == [-64, 0, 10, 74]
    for bad in ([-65], [75], [2 ** 31 - 1], [-2 ** 31]):
        with pytest.raises(AssertionError):
            G.bounded(bad, 0, 10, 16)
    assert G.bounded([-32], 0, 10, 128).tolist() == [-32]
    with pytest.raises(AssertionError):
        G.bounded([-33], 0, 10, 128)                                        # 33 rows of 128 B leave a 4 KiB guard
    with pytest.raises(AssertionError):
        G.bounded([11], 0, 10, 8192)                                        # no such row fits the guard at all
    assert G.bounded([-2, 5], 0, 10, 4096, guard_bytes=8192).tolist() == [-2, 5]
    assert G.bounded([], 0, 10, 16).size == 0


def test_refill_and_write_move_the_reference():
    ws = Buf(16, torch.uint8, device="cpu")
    ws.refill(0x00)
    assert ws.untouched() and ws.body().tolist() == [0] * 16 and ws.guards_intact()
    ws.refill(0xFF)
    assert ws.untouched() and bool(ws.poisoned().all())
    ws.write(np.arange(16, dtype=np.uint8))
    assert ws.untouched() and ws.body().tolist() == list(range(16))


def _finished_call(written, values, dtype=torch.float64, fill="poison"):
    """a Call whose one output `y` [6] a "kernel" has written `values` into, at the entries of `written`"""
    c = A.Call("cpu_kernel")
    c.outs["y"] = Buf(6, dtype, fill=fill, device="cpu")
    v = _body_view(c.outs["y"])
    for i, x in zip(written, values):
        v[i] = x
    return c


def test_expect_accepts_a_clean_call_and_fails_in_three_ways():
    want = np.array([1.0, 2.0, 3.0, 4.0, 0.0, 0.0])
    rows = np.arange(6) < 4                                                # "entries 4 and 5 are not written"
    A.expect(_finished_call(range(4), want), "y", want, rows)
    A.expect(_finished_call(range(6), want), "y", want)
    A.expect(_finished_call(range(4), [1.0, np.nan, 3.0, -0.0]), "y", [1.0, np.nan, 3.0, -0.0, 9.0, 9.0], rows)
    # an entry that should be written still holds the fill
    with pytest.raises(AssertionError, match="1 entries the header says are written still hold the fill pattern"):
        A.expect(_finished_call([0, 1, 3], [1.0, 2.0, 4.0]), "y", want, rows)
    # an entry outside `written` changed
    with pytest.raises(AssertionError, match="1 entries written that the header says are not written"):
        A.expect(_finished_call(range(5), want), "y", want, rows)
    # a NaN stands where a number is wanted (and the other way round; and the poison's own bits, written by the kernel)
    with pytest.raises(AssertionError, match=r"1 entries differ, first at \[\[2\]\]"):
        A.expect(_finished_call(range(4), [1.0, 2.0, np.nan, 4.0]), "y", want, rows)
    with pytest.raises(AssertionError, match="1 entries differ"):
        A.expect(_finished_call(range(4), want), "y", [1.0, 2.0, np.nan, 4.0, 0.0, 0.0], rows)
    with pytest.raises(AssertionError, match="still hold the fill pattern"):
        A.expect(_finished_call(range(4), [1.0, 2.0, A.POISON64, 4.0]), "y", [1.0, 2.0, np.nan, 4.0, 0.0, 0.0], rows)
    # under a `close` the comparison is the caller's, the placement checks stay
    seen = []
    A.expect(_finished_call(range(4), want), "y", want + 0.5, rows, close=lambda g, w, what: seen.append((g.tolist(), w.tolist())))
    assert seen == [([1.0, 2.0, 3.0, 4.0], [1.5, 2.5, 3.5, 4.5])]
    with pytest.raises(AssertionError, match="still hold the fill pattern"):
        A.expect(_finished_call([0, 1, 3], [1.0, 2.0, 4.0]), "y", want, rows, close=lambda g, w, what: None)
    # int32 outputs in which -1 is legal start as garbage: a written -1 is a value, an unwritten entry is not
    ids = _finished_call(range(6), [3, -1, 0, -1, 2, -1], torch.int32, "garbage")
    A.expect(ids, "y", [3, -1, 0, -1, 2, -1])
    with pytest.raises(AssertionError, match="still hold the fill pattern"):
        A.expect(_finished_call(range(5), [3, -1, 0, -1, 2], torch.int32, "garbage"), "y", [3, -1, 0, -1, 2, -1])
    A.check_all(ids, {"y": [3, -1, 0, -1, 2, -1]})
    with pytest.raises(AssertionError, match="entries differ"):
        A.check_all(ids, {"y": [3, -1, 0, -1, 2, 0]})


def test_bits_equal_tells_zero_signs_and_treats_all_nans_as_one_value():
    assert A.bits_equal(np.array([0.0, 1.5]), np.array([0.0, 1.5]))
    assert not A.bits_equal(np.array([0.0, 1.5]), np.array([-0.0, 1.5]))
    quiet, negative, payload = np.nan, -np.nan, np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), np.float64)[0]
    assert A.bits_equal(np.array([quiet, 2.0]), np.array([negative, 2.0])) and A.bits_equal(np.array([quiet]), np.array([payload]))
    assert A.bits_equal(np.array([quiet]), np.array([A.POISON64])) and not G.same_bits(np.array([quiet]), np.array([A.POISON64]))
    assert not A.bits_equal(np.array([np.nan, 2.0]), np.array([2.0, np.nan]))             # the NaNs stand in different places
    assert not A.bits_equal(np.array([np.nan]), np.array([np.inf]))
    assert not A.bits_equal(np.zeros(2, np.float32), np.zeros(2, np.float64)) and not A.bits_equal(np.zeros(2), np.zeros(3))
    assert A.bits_equal(np.array([3, -1], np.int32), np.array([3, -1], np.int32))
    assert not A.bits_equal(np.array([3, -1], np.int32), np.array([3, 0], np.int32))
    a, b = _finished_call(range(6), [1.0, np.nan, -0.0, 4.0, 5.0, 6.0]), _finished_call(range(6), [1.0, -np.nan, -0.0, 4.0, 5.0, 6.0])
    A.same_results(a, b)
    with pytest.raises(AssertionError, match="y differs between the two runs"):
        A.same_results(a, _finished_call(range(6), [1.0, np.nan, 0.0, 4.0, 5.0, 6.0]))


def test_sanitise_csr_is_the_header_sentence():
    assert A.sanitise_csr([-3, 2, 1, 9, 12], 10) == [(0, 2), (2, 2), (1, 9), (9, 10)]
    assert A.sanitise_csr([13, 4], 10) == [(10, 10)]
