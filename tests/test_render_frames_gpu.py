"""GPU half of the single-particle renderer's suite: mivit_render_frames (csrc/render.hip) and its caller
helpers/generation.render_frames against the fp64 reference, per pixel, with the measured bar of tests/render_common.py;
placement through the C-ABI inside guarded allocations; independence, symmetry and one-hot properties, bitwise where the
arithmetic allows it; the caller's 65 535-sequence chunk loop; the wrapper's input handling; the launcher's rejections;
trajectories_to_video with the noise turned off."""
import ctypes

import numpy as np
import pytest
import torch

import render_common as rc

pytestmark = pytest.mark.gpu

IDS = [c["id"] for c in rc.cases()]
WORST = {}


def gen():
    from moleculardiffusion_mivit_amd.helpers import generation
    return generation


def nat():
    from moleculardiffusion_mivit_amd import _native
    return _native


def render(traj, npos, sigmas, P, up, amp, center=False):
    """numpy or tensors in -> the wrapper on the device -> CPU tensor"""
    t = torch.as_tensor(traj).cuda()
    a = torch.as_tensor(amp).cuda()
    out = gen().render_frames(t, npos, sigmas, P, up, a, center)
    torch.cuda.synchronize()
    assert out.is_cuda
    return out.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def rand_case(seed, N, F, npos, P):
    rng = np.random.default_rng(seed)
    return rc._traj(rng, N, F, npos, P), rc._amps(rng, N, F, npos)


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_every_table_entry_meets_the_per_pixel_bar(cid):
    """Measured on the MI355X, worst error / bar: grid 0.25, npos 0.29, nsig 0.31, amps 0.25, ties 0.24, far-narrow 0.31,
    far-wide 0.28, straddle 0.31, lds 0.25; at most 7e-7 of a case's maximum.  With d*d - dpk*dpk in the kernel:
    far-9x5-wide-A / -B 4.3 / 3.8 and the brightest pixels of far-*-narrow 1.5e-5 of the maximum."""
    c, rec = rc.case(cid), rc.table()[cid]
    got = render(*rc.args(c)).numpy()
    assert got.dtype == np.float32 and got.shape == rec["ref"].shape and np.isfinite(got).all()
    r, err, b, i = rc.ratio(got, rec["ref"], rc.bar(cid))
    ok, rel = rc.outer_ok(got, rec["ref"])
    WORST[cid] = r
    print(f"RENDER {cid} group {c['group']} ratio {r:.3f} err {err:.3e} bar {b:.3e} outer {rel:.2e} c_arg {rc.c_arg(cid):.3e}")
    assert r <= 1.0 and ok


# ---- 2. placement through the C-ABI -----------------------------------------------------------------------------------
def call_abi(traj, npos, sigmas, P, up, amp, center, guard=512):
    """-> (return code, body, guards intact).  out inside a NaN-filled allocation with `guard` floats on both sides, traj
    and amp 16 bytes into NaN-filled allocations that end with one more NaN"""
    traj, amp = torch.as_tensor(traj), torch.as_tensor(amp)
    N, T, _ = traj.shape
    F, nsig = T // npos, len(sigmas)
    n_out = N * nsig * F * P * P
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    raw = torch.full((guard + n_out + guard,), float("nan"), device="cuda")
    tbuf = torch.full((4 + traj.numel() + 1,), float("nan"), device="cuda")
    abuf = torch.full((4 + amp.numel() + 1,), float("nan"), device="cuda")
    tbuf[4:4 + traj.numel()] = traj.reshape(-1).cuda()
    abuf[4:4 + amp.numel()] = amp.reshape(-1).cuda()
    sig = torch.tensor(sigmas, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)      # noqa: E731
    rcode = nat().lib.mivit_render_frames(p(tbuf, 4), N, T, npos, p(sig), nsig, P, up, p(abuf, 4), int(center), p(raw, guard),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    flat = raw.cpu()
    g = torch.cat([flat[:guard], flat[guard + n_out:]])
    return rcode, flat[guard:guard + n_out].view(N, nsig, F, P, P), bool((bits(g) == nan_bits).all())


@pytest.mark.parametrize("N,F,npos,nsig,P,up", [(3, 2, 2, 2, 9, 5), (2, 1, 3, 1, 64, 5)])
def test_placement_inside_guarded_allocations(N, F, npos, nsig, P, up):
    traj, amp = rand_case(7 + P, N, F, npos, P)
    sigmas = rc.sig32(*np.linspace(1.1 * up, 0.5 * up, nsig))
    rcode, body, guards = call_abi(traj, npos, sigmas, P, up, amp, True)
    assert rcode == 0, nat().last_error()
    assert bool(torch.isfinite(body).all()) and guards
    assert same(body, render(traj, npos, sigmas, P, up, amp, True))


# ---- 3. independence and repeatability ---------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [False, True])
def test_batch_frame_and_sigma_independence_bitwise(center):
    N, F, npos, P, up = 4, 3, 5, 9, 5
    traj, amp = rand_case(11, N, F, npos, P)
    sig = rc.sig32(2.3, 1.5, 7.0)
    whole = render(traj, npos, sig, P, up, amp, center)
    assert same(whole, render(traj, npos, sig, P, up, amp, center))                        # two launches
    for n in range(N):                                                                       # a sequence alone
        assert same(whole[n:n + 1], render(traj[n:n + 1], npos, sig, P, up, amp[n:n + 1], center))
    perm = [2, 0, 3, 1]
    assert same(whole[perm], render(traj[perm], npos, sig, P, up, amp[perm], center))       # a permuted batch
    # every frame as a trajectory of its own: the centre is per frame, so center=True is bitwise as well
    frames = render(traj.reshape(N * F, npos, 2), npos, sig, P, up, amp.reshape(N * F, 1, npos), center)
    assert same(whole.permute(0, 2, 1, 3, 4).reshape(N * F, len(sig), 1, P, P), frames)
    for si, s in enumerate(sig):                                                             # every sigma alone
        assert same(whole[:, si:si + 1], render(traj, npos, [s], P, up, amp, center))


# ---- 4. symmetry -------------------------------------------------------------------------------------------------------
def test_a_centred_spot_is_symmetric_and_x_is_the_last_axis():
    sig = rc.sig32(0.8, 2.3)
    zero = np.zeros((1, 1, 2), np.float32)
    one = np.ones((1, 1, 1), np.float32)
    # Amplitude 1 throughout: the kernel multiplies (a py[y]) px[x], and only a power of two commutes with the rounding of
    # that product, so with a = 500 the transpose of an exactly symmetric pair of profiles differs in the last bit.
    # up = 1: a pixel is one exponential, so mirrored pixels hold the same number
    fr = render(zero, 1, sig, 9, 1, one)
    assert float(fr.max()) == 1.0 and same(fr, fr.transpose(-1, -2)) and same(fr, fr.flip(-1)) and same(fr, fr.flip(-2))
    # up = 5, odd G: rows and columns are computed by the same code, so the transpose is bitwise; a mirrored pixel sums the
    # same five exponentials in the opposite order: each sum is within up - 1 roundings of the exact one, and the division
    # and the two products add three more on either side
    fr = render(zero, 1, sig, 9, 5, one)
    assert same(fr, fr.transpose(-1, -2))
    for flipped in (fr.flip(-1), fr.flip(-2)):
        assert bool(((fr - flipped).abs() <= (2 * (5 - 1) + 6) * rc.U32 * fr.abs()).all())
    # swapping the columns of an off-centre trajectory transposes the frame
    traj = np.array([[[1.3, -0.4], [2.1, 0.7], [-0.6, 3.2]]], np.float32)
    fr = render(traj, 3, sig, 9, 5, np.ones((1, 1, 3), np.float32))
    sw = render(traj[..., ::-1].copy(), 3, sig, 9, 5, np.ones((1, 1, 3), np.float32))
    assert same(sw, fr.transpose(-1, -2)) and not same(sw, fr)
    # a displacement in +x moves the centroid along the last axis only, towards larger indices
    fr = render(np.array([[[1.5, 0.0]]], np.float32), 1, sig, 9, 5, one)[0, 1, 0].double()
    idx = torch.arange(9, dtype=torch.float64)
    cy, cx = float((fr.sum(1) * idx).sum() / fr.sum()), float((fr.sum(0) * idx).sum() / fr.sum())
    assert abs(cy - 4.0) < 1e-6 and 5.0 < cx < 6.0


# ---- 5. one-hot amplitudes ---------------------------------------------------------------------------------------------
def test_one_hot_amplitudes_give_the_outer_product_and_sum_to_the_full_render():
    P, up, npos = 9, 5, 5
    c = rc.case("straddle-9x5")                        # sub-positions inside and far outside: the reference underflows for some
    traj, sig = c["traj"][:1], rc.sig32(rc.NARROW * up, 2.3)
    amp = np.abs(c["amp"][:1])
    full = render(traj, npos, sig, P, up, amp)
    acc = torch.zeros_like(full)
    mag = torch.zeros_like(full)
    zeros = 0
    for p in range(npos):
        hot = np.zeros_like(amp)
        hot[..., p] = amp[..., p]
        got = render(traj, npos, sig, P, up, hot)
        ref, bar = rc.bar_for(traj, npos, sig, P, up, hot, False)
        # the product of this sub-position's two profiles: the reference with one spot
        prof, _ = rc.profiles64(traj, npos, sig, P, up, False)
        outer = hot[0, 0, p] * prof[:, :, :, p, 1, :, None] * prof[:, :, :, p, 0, None, :]
        assert (np.abs(outer - ref) <= 1e-12 * np.abs(outer) + 1024 * rc.ref_floor(hot, rc.reference(traj, npos, sig, P, up, hot, False)[1])).all()
        assert rc.ratio(got.numpy(), ref, bar)[0] <= 1.0
        under = torch.from_numpy(ref == 0)
        zeros += int(under.sum())
        assert bool((got[under] == 0).all())
        acc = acc + got                                 # sequential fp32 sum, p ascending: the kernel's order without FMA
        mag = mag + got.abs()
    assert zeros > 0
    # 2 ulp: the compiler may contract the kernel's multiply-add, which then rounds a term once instead of twice
    assert bool(((full - acc).abs() <= 2 * (2 * rc.U32) * mag).all())


# ---- 6. the caller's chunk loop ----------------------------------------------------------------------------------------
def test_chunk_loop_past_65535_sequences():
    N = rc.MAX_GRID + 3
    rng = np.random.default_rng(5)
    traj = rng.uniform(-1.5, 1.5, (N, 1, 2)).astype(np.float32)
    amp = (100 + rng.uniform(0, 50, (N, 1, 1))).astype(np.float32)
    sig = rc.sig32(0.8)
    out = render(traj, 1, sig, 3, 1, amp)
    assert out.shape == (N, 1, 1, 3, 3) and bool(torch.isfinite(out).all())
    for n in (0, rc.MAX_GRID - 1, rc.MAX_GRID, N - 1):
        assert same(out[n:n + 1], render(traj[n:n + 1], 1, sig, 3, 1, amp[n:n + 1])), n
    ref, _ = rc.reference(traj[-4:], 1, sig, 3, 1, amp[-4:], False)
    assert np.abs(out[-4:].numpy() - ref).max() < rc.OUTER * np.abs(ref).max()


# ---- 7. wrapper inputs -------------------------------------------------------------------------------------------------
def test_wrapper_handles_strides_broadcast_amplitudes_fp64_and_cpu_amplitudes():
    G = gen()
    N, F, npos, P, up = 3, 2, 4, 9, 5
    traj, amp = rand_case(21, N, F, npos, P)
    sig = rc.sig32(2.3, 1.1)
    want = render(traj, npos, sig, P, up, amp, True)
    t, a = torch.from_numpy(traj).cuda(), torch.from_numpy(amp).cuda()
    # non-unit strides: swapped columns of a swapped copy, and a slice of a longer, wider tensor
    view = t[..., [1, 0]].contiguous()[..., [1, 0]]
    big = torch.full((N, F * npos + 3, 5), float("nan"), device="cuda")
    big[:, 2:2 + F * npos, 1:3] = t
    flipped = t.flip(-1).flip(-1)
    tt = t.transpose(0, 1).contiguous().transpose(0, 1)
    for v in (view, big[:, 2:2 + F * npos, 1:3], flipped, tt):
        assert torch.equal(v, t)
        assert same(G.render_frames(v, npos, sig, P, up, a, True).cpu(), want)
    assert not big[:, 2:2 + F * npos, 1:3].is_contiguous() and not tt.is_contiguous()
    # broadcast amplitudes
    a_f = a[:, :, :1].contiguous()
    assert same(G.render_frames(t, npos, sig, P, up, a_f, True).cpu(), render(traj, npos, sig, P, up, a_f.expand(N, F, npos).contiguous(), True))
    a_p = a[:1, :1, :].contiguous()
    assert same(G.render_frames(t, npos, sig, P, up, a_p, True).cpu(), render(traj, npos, sig, P, up, a_p.expand(N, F, npos).contiguous(), True))
    # spot_intensity on the CPU
    assert same(G.render_frames(t, npos, sig, P, up, torch.from_numpy(amp), True).cpu(), want)
    # an fp64 trajectory (holding fp32 values, so that the kernel reads what the reference reads) returns fp64
    out = G.render_frames(t.double(), npos, sig, P, up, a.double(), True)
    assert out.dtype == torch.float64 and out.is_cuda and torch.equal(out.cpu(), want.double())
    ref, bar = rc.bar_for(traj, npos, sig, P, up, amp, True)
    assert rc.ratio(out.cpu().numpy(), ref, bar)[0] <= 1.0


# ---- 8. rejections -----------------------------------------------------------------------------------------------------
def test_launcher_rejections_and_the_lds_boundary():
    N_ = nat()
    buf = torch.zeros(1 << 16, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    null = ctypes.c_void_p(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(traj=p, N=1, T=2, npos=2, sig=p, nsig=1, P=3, up=1, amp=p, out=p):
        return N_.lib.mivit_render_frames(traj, N, T, npos, sig, nsig, P, up, amp, 0, out, st)

    def rejected(msg, **kw):
        assert call(**kw) != 0, kw
        assert msg in N_.last_error(), (kw, N_.last_error())

    for name in ("traj", "sig", "amp", "out"):
        rejected("null pointer", **{name: null})
    for name in ("N", "T", "npos", "nsig", "P", "up"):
        rejected("empty problem", **{name: 0})
    rejected("divisble", T=5, npos=2)
    rejected("65535", N=rc.MAX_GRID + 1)
    rejected("65535", nsig=rc.MAX_GRID + 1)
    n_max = rc.lds_max_npos(64)
    rejected("do not fit LDS", T=n_max + 1, npos=n_max + 1, P=64)
    torch.cuda.synchronize()
    assert bool((buf == 0).all())                      # a rejected call launches nothing
    # the largest accepted npos runs, through the C-ABI inside guards, and is the table entry the accuracy test judges
    c = rc.case("lds-64x5")
    assert c["npos"] == n_max
    rcode, body, guards = call_abi(*rc.args(c))
    assert rcode == 0 and guards
    assert rc.ratio(body.numpy(), rc.table()["lds-64x5"]["ref"], rc.bar("lds-64x5"))[0] <= 1.0


# ---- 9. the data path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [False, True])
def test_trajectories_to_video_without_noise(center):
    """background_intensity [b, 0] and poisson_noise -1 leave frames + b.  The amplitudes are drawn inside, on the device of
    the call, so they cannot be shared between a CPU and a CUDA call: with std <= 1e-4 both take the zero-amplitude branch and
    must agree exactly; with a drawn amplitude each side is compared with the reference fed the same draw (the first of the
    generator) and the trajectory transformed by hand."""
    G = gen()
    N, F, npos, P, up = 3, 2, 5, 9, 5
    b = 100.0
    rng = np.random.default_rng(31)
    traj = (rng.uniform(-2.0, 2.0, (N, F, 1, 2)) + 0.3 * rng.standard_normal((N, F, npos, 2))).reshape(N, F * npos, 2).astype(np.float32)
    props = {"output_size": P, "upsampling_factor": up, "background_intensity": [b, 0], "poisson_noise": -1,
             "trajectory_unit": 64, "resolution": 128e-9}          # a scaling by exactly 1 / 2, however the division is carried out
    sig = rc.sig32(G.psf_sigma_hr({**G.DEFAULT_IMAGE_PROPS, **props}))
    # zero-amplitude branch: CUDA equals CPU, both exactly the background
    props0 = dict(props, particle_intensity=[500.0, 5e-5])
    t_dev = torch.from_numpy(traj).cuda()
    keep = t_dev.clone()
    v_gpu = G.trajectories_to_video(t_dev, npos, center, props0)
    v_cpu = G.trajectories_to_video(torch.from_numpy(traj), npos, center, props0)
    assert v_gpu.is_cuda and v_gpu.dtype == torch.float32 and v_gpu.shape == (N, F, P, P)
    assert torch.equal(v_gpu.cpu(), v_cpu) and bool((v_cpu == b).all())
    assert torch.equal(t_dev, keep)
    # drawn amplitudes: the y flip and the unit scaling applied once
    props1 = dict(props, particle_intensity=[500.0, 20.0])
    by_hand = (traj * np.array([1.0, -1.0], np.float32)) * np.float32(64) / np.float32(128e-9 * 1e9)
    assert np.array_equal(by_hand, traj * np.array([0.5, -0.5], np.float32))
    for dev in ("cuda", "cpu"):
        g1, g2 = torch.Generator(device=dev).manual_seed(9), torch.Generator(device=dev).manual_seed(9)
        t_in = torch.from_numpy(traj).to(dev)
        keep = t_in.clone()
        vid = G.trajectories_to_video(t_in, npos, center, props1, generator=g1)
        assert torch.equal(t_in, keep) and vid.device.type == dev
        amp = (500.0 / npos + (20.0 / npos) * torch.randn(N, F, npos, generator=g2, device=dev)).cpu().numpy()
        assert np.array_equal(np.float32(by_hand), by_hand) and by_hand.dtype == np.float32
        ref, bar = rc.bar_for(by_hand, npos, sig, P, up, amp, center)
        ref, bar = ref[:, 0] + b, bar[:, 0] + 2 * rc.U32 * (np.abs(ref[:, 0]) + b)      # + one rounding of the frame, one of the sum
        r = rc.ratio(vid.cpu().numpy(), ref, bar)
        print(f"RENDER video {dev} center={center}: worst error / bar {r[0]:.3f}")
        assert r[0] <= 1.0
        unflipped, _ = rc.reference(by_hand * np.array([1.0, -1.0], np.float32), npos, sig, P, up, amp, center)
        assert rc.ratio(vid.cpu().numpy(), unflipped[:, 0] + b, bar)[0] > 100             # the flip matters at this bar
