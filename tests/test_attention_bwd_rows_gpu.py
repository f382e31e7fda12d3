"""mivit_attention_bwd_rows (the attention-core backward told how many query rows of a sequence carry a gradient) against
mivit_attention_bwd on the zero-padded dctx.  The full kernel is the authority: tests/test_attention_core_gpu.py pins it to fp64.

The compact dctx is exactly B * q_rows * E elements long inside a guarded allocation (a read of a row >= q_rows of the last
sequence leaves the region; inside it, it would pick up the next sequence's gradient and change the result), dqkv starts as NaN:
all of it must be written and equal, as values, what the full kernel makes of the padded problem."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H = 3, 4
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
PATTERN = 0xA5
CASES = [(S, Dh, q) for S in (1, 2, 16, 17, 33, 48, 64) for Dh in (16, 32) for q in sorted({1, min(S, 16), min(S, 17), S})]


def _native():
    from moleculardiffusion_mivit_amd import _native as N
    return N


def _guarded(numel, dtype):
    """`numel` elements between 256 bytes and 4 KiB of a byte pattern -> (whole allocation, view of the region)"""
    nbytes = numel * 2
    raw = torch.full((256 + nbytes + 4096,), PATTERN, dtype=torch.uint8, device="cuda")
    return raw, raw[256:256 + nbytes].view(dtype)


def _intact(raw, numel):
    return bool((raw[:256] == PATTERN).all()) and bool((raw[256 + numel * 2:] == PATTERN).all())


@pytest.mark.parametrize("precision", sorted(DT))
@pytest.mark.parametrize("S,Dh,q_rows", CASES)
def test_rows_entry_equals_full_kernel_on_padded_dctx(S, Dh, q_rows, precision):
    N = _native()
    dt, code = DT[precision], {"bf16": N.BF16, "fp16": N.F16}[precision]
    E = H * Dh
    g = torch.Generator().manual_seed(1000 * S + 10 * Dh + q_rows)
    qkv = torch.randn(B, S, 3 * E, generator=g).to(dt).cuda()
    d = torch.randn(B, q_rows, E, generator=g).to(dt)
    craw, compact = _guarded(B * q_rows * E, dt)
    compact.copy_(d.reshape(-1))
    padded = torch.zeros(B, S, E, dtype=dt)
    padded[:, :q_rows] = d
    padded = padded.cuda()
    oraw, got = _guarded(B * S * 3 * E, dt)
    fraw, full = _guarded(B * S * 3 * E, dt)
    got.fill_(float("nan"))
    full.fill_(float("nan"))
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib.mivit_attention_bwd(code, p(qkv), p(padded), B, S, H, Dh, p(full), st), "attention_bwd")
    N.check(N.lib.mivit_attention_bwd_rows(code, p(qkv), p(compact), q_rows * E, q_rows, B, S, H, Dh, p(got), st), "attention_bwd_rows")
    torch.cuda.synchronize()
    assert _intact(craw, B * q_rows * E) and _intact(oraw, B * S * 3 * E) and _intact(fraw, B * S * 3 * E)
    assert bool(torch.isfinite(full.float()).all())
    assert bool(torch.isfinite(got.float()).all()), "an element of dqkv was not written"
    assert torch.equal(got.float(), full.float())          # values: the sign of a zero is not compared
    if q_rows < S:                                         # dq of the rows without a gradient: zeros
        assert bool((got.view(B, S, 3 * E)[:, q_rows:, :E].float() == 0).all())


def test_rows_entry_rejects_bad_row_counts():
    """host-side checks only: no kernel is launched for q_rows outside 1..S, a stride shorter than the rows, or fp32"""
    N = _native()
    t = torch.zeros(4096, dtype=torch.bfloat16, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    for dtype, stride, q in ((N.BF16, 64, 0), (N.BF16, 64, 3), (N.BF16, 32, 1), (N.F32, 64, 1)):
        assert N.lib.mivit_attention_bwd_rows(dtype, p, p, stride, q, 1, 2, 4, 16, p, None) != 0, (dtype, stride, q)
