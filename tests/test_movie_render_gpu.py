"""GPU half of the whole-field renderer's suite: mivit_render_movie (csrc/movie.hip) and its callers
helpers/generation.render_movie and simulate_movie(device="cuda") against the fp64 reference, per pixel, with the measured bar
of tests/movie_common.py; placement through the C-ABI inside guarded allocations; bitwise properties (repeatability, a frame
alone, lifetimes against a sliced particle list, insertion of particles that contribute nothing, one-hot pairs, flip symmetry);
the wrapper's input handling; the simulator on the device.

Measured on the MI355X, worst error / bar per group: grid 0.41, npos 0.26, chunk 0.16, batch 0.21, cull 0.20, ring 0.15,
amps 0.24, ties 0.22, nonfinite 0.19, lifetimes 0.19, far 0.09; simulate_movie 0.40; at most 1.0e-6 of a case's maximum.
Run time there: 95 tests in 4.7 s; the slowest is the first accuracy case, 0.95 s, which computes the table's references once
(every other test takes at most 0.5 s).  Nothing failed, so csrc/movie.hip is unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import movie_common as mc

pytestmark = pytest.mark.gpu

IDS = [c["id"] for c in mc.cases()]
WORST = {}


def gen():
    from moleculardiffusion_mivit_amd.helpers import generation
    return generation


def ops():
    from moleculardiffusion_mivit_amd import ops as o
    return o


def nat():
    from moleculardiffusion_mivit_amd import _native
    return _native


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).cuda()


def render(c, pos=None, amp=None, first="case", last="case", H=None, W=None):
    """a case (or parts of it replaced) -> the wrapper on the device -> CPU fp32 tensor [F, H, W]"""
    first = c["first"] if isinstance(first, str) else first
    last = c["last"] if isinstance(last, str) else last
    out = gen().render_movie(dev(c["pos"] if pos is None else pos), dev(c["amp"] if amp is None else amp), c["sigma"], H or c["H"],
                             W or c["W"], c["up"], c["radius"], dev(first), dev(last))
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.float32
    return out.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def make(H, W, up, sigma, radius, pos, amp, first=None, last=None):
    return mc._case("adhoc", "adhoc", H, W, up, sigma, radius, pos, amp, first, last)


# ---- 1. accuracy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_every_table_entry_meets_the_per_pixel_bar(cid):
    c, rec = mc.case(cid), mc.table()[cid]
    got = render(c).numpy()
    assert got.shape == rec["ref"].shape and np.isfinite(got).all()
    r, err, b, i = mc.ratio(got, rec["ref"], mc.bar(cid))
    ok, rel = mc.outer_ok(got, rec["ref"])
    WORST[c["group"]] = max(WORST.get(c["group"], 0.0), r)
    print(f"MOVIE {cid} group {c['group']} ratio {r:.3f} err {err:.3e} bar {b:.3e} outer {rel:.2e} c_arg {mc.c_arg(cid) / mc.U32:.2f} "
          f"yardstick-equal pixels {float((got == rec['yard'].astype(np.float32)).mean()):.3f}")
    assert r < 1.0 and ok
    assert (got[rec["ref"] == 0] == 0).all()                     # nothing outside the windows, nothing from what contributes nothing


def test_worst_ratio_per_group():
    """prints what the accuracy test collected (nothing when it runs alone)"""
    for g in sorted(WORST):
        print(f"MOVIE-GROUP {g} worst error / bar {WORST[g]:.3f}")
    assert all(v < 1.0 for v in WORST.values())


def test_far_field_is_bitwise_the_scene_at_the_origin():
    """c - rint(c) is exact and nothing after it sees the size of the coordinate: the claim of the kernel's header"""
    far, org = render(mc.case("far-2^20")), render(mc.case("far-origin"))
    for a, b in mc.far_regions():
        assert float(org[:, :, b].max()) > 1 and same(far[:, :, a], org[:, :, b])
    lit = torch.zeros(far.shape[-1], dtype=torch.bool)
    for a, _ in mc.far_regions():
        lit[a] = True
    assert bool((far[:, :, ~lit] == 0).all())


# ---- 2. placement through the C-ABI -------------------------------------------------------------------------------------
GUARD = 4096


def test_placement_inside_guarded_allocations():
    """movie between NaN guards; pos and amp 16 bytes into NaN-filled allocations with a NaN behind their last element; first
    and last likewise between sentinels (first 0, last 1000) that would make a neighbouring particle visible in every frame"""
    c = mc.case("lifetimes")
    Np, F, npos, H, W = c["Np"], c["F"], c["npos"], 37, 70
    n_out = F * H * W
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    raw = torch.full((GUARD + n_out + GUARD,), float("nan"), device="cuda")
    pbuf = torch.full((4 + c["pos"].size + 1,), float("nan"), device="cuda")
    abuf = torch.full((4 + c["amp"].size + 1,), float("nan"), device="cuda")
    fbuf = torch.zeros(4 + Np + 1, dtype=torch.int32, device="cuda")
    lbuf = torch.full((4 + Np + 1,), 1000, dtype=torch.int32, device="cuda")
    pbuf[4:-1] = dev(c["pos"]).reshape(-1)
    abuf[4:-1] = dev(c["amp"]).reshape(-1)
    fbuf[4:-1] = dev(c["first"])
    lbuf[4:-1] = dev(c["last"])
    p = lambda t, off: ctypes.c_void_p(t.data_ptr() + 4 * off)      # noqa: E731
    rcode = nat().lib.mivit_render_movie(p(pbuf, 4), p(abuf, 4), p(fbuf, 4), p(lbuf, 4), Np, F, npos, c["sigma"], c["up"], c["radius"],
                                        H, W, p(raw, GUARD), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rcode == 0, nat().last_error()
    flat = raw.cpu()
    guards = torch.cat([flat[:GUARD], flat[GUARD + n_out:]])
    assert bool((bits(guards) == nan_bits).all())
    body = flat[GUARD:GUARD + n_out].view(F, H, W)
    assert bool(torch.isfinite(body).all())
    want = ops().render_movie(dev(c["pos"]), dev(c["amp"]), c["sigma"], c["up"], c["radius"], H, W, dev(c["first"]), dev(c["last"]))
    assert same(body, want.cpu())
    assert mc.ratio(body.numpy(), mc.table()["lifetimes"]["ref"], mc.bar("lifetimes"))[0] < 1.0


# ---- 3. bitwise ---------------------------------------------------------------------------------------------------------
def test_two_launches_a_frame_alone_and_lifetimes_against_a_sliced_list():
    c = mc.case("lifetimes")
    F, npos = c["F"], c["npos"]
    whole = render(c)
    assert same(whole, render(c))
    for f in range(F):
        sl = slice(f * npos, (f + 1) * npos)
        alone = render(c, pos=c["pos"][:, sl], amp=c["amp"][:, f:f + 1], first=c["first"] - f, last=c["last"] - f)
        assert same(alone[0], whole[f]), f
        keep = (c["first"] <= f) & (f <= c["last"])              # the particle list sliced to those visible in frame f
        assert 0 < keep.sum() < c["Np"]
        sliced = render(c, pos=c["pos"][keep][:, sl], amp=c["amp"][keep][:, f:f + 1], first=None, last=None)
        assert same(sliced[0], whole[f]), f
    # the same without any lifetimes: a frame alone is the frame of the movie
    c = mc.case("npos-5")
    whole = render(c)
    for f in range(c["F"]):
        assert same(render(c, pos=c["pos"][:, f * 5:(f + 1) * 5], amp=c["amp"][:, f:f + 1])[0], whole[f])


def test_particles_that_contribute_nothing_change_no_bit_wherever_they_stand():
    """invisible by lifetime, non-finite, wholly outside the field: in front, in the middle and at the end of the list, which
    moves every real pair to another thread, another survivor index and, with 250 of them, another pass of the chunk loop"""
    c = mc.case("npos-5")
    Np, F, npos = c["Np"], c["F"], c["npos"]
    first, last = np.zeros(Np, np.int32), np.full(Np, F - 1, np.int32)
    base = render(c, first=first, last=last)
    assert same(base, render(c))
    rng = np.random.default_rng(3)
    T = F * npos
    inside = rng.uniform([3, 3], [33, 66], (1, T, 2)).astype(np.float32)
    nothing = {
        "invisible": (inside, F + 1, F + 1),
        "nan": (np.full((1, T, 2), np.nan, np.float32), 0, F - 1),
        "inf": (inside * np.array([np.inf, 1], np.float32), 0, F - 1),
        "outside": (inside + np.float32(500), 0, F - 1),
        "huge": (np.full((1, T, 2), -mc.BELOW_MAX_COORD, np.float32), 0, F - 1),
    }
    amp1 = np.full((1, F, npos), 1e4, np.float32)
    for name, (pz, fz, lz) in nothing.items():
        for where, reps in ((0, 1), (Np // 2, 1), (Np, 1), (0, 250), (Np // 2, 250)):
            pos = np.concatenate([c["pos"][:where]] + [pz] * reps + [c["pos"][where:]])
            amp = np.concatenate([c["amp"][:where]] + [amp1] * reps + [c["amp"][where:]])
            fi = np.concatenate([first[:where], np.full(reps, fz, np.int32), first[where:]])
            la = np.concatenate([last[:where], np.full(reps, lz, np.int32), last[where:]])
            assert same(render(c, pos=pos, amp=amp, first=fi, last=la), base), (name, where, reps)


def test_one_hot_pair_is_the_rounded_product_of_its_two_profiles():
    """up = 1, where an integer coordinate has the profile value exactly 1 on its own pixel: py is read from an amplitude-1
    render at (cy, integer), px from one at (integer, cx), and a single pair of amplitude a must give fl(fl(a py[y]) px[x])
    bit for bit.  Also prints, per sigma, how many peak pixels of the fractional positions are exactly 1: with d*d - dpk*dpk
    contracted into fma(d, d, -fl(dpk^2)) the peak sample's argument is the rounding error of dpk^2 times inv2s2 instead of 0,
    at most 2^-26 inv2s2, which shows once inv2s2 is large (sigma_hr = 0.1: 50).  Either way each profile
    must meet the bar, whose FMA term is this very quantity."""
    H, W, r = 37, 70, 3
    rng = np.random.default_rng(17)
    for sigma in (0.1, 0.3, 0.8):
        peaks = exact = 0
        for cy, cx in rng.uniform([4, 4], [32, 65], (6, 2)).astype(np.float32):
            iy, ix = int(np.rint(cy)), int(np.rint(cx))
            one = np.ones((1, 1, 1), np.float32)
            a = np.float32(137.3)
            both = render(make(H, W, 1, sigma, r, [[[cy, cx]]], one * a))[0]
            col = render(make(H, W, 1, sigma, r, [[[cy, np.float32(ix)]]], one))[0]
            row = render(make(H, W, 1, sigma, r, [[[np.float32(iy), cx]]], one))[0]
            # the peak sample: exp(0) = 1 unfused; contracted, exp of at most 2^-26 inv2s2 either way (movie_common's FMA term),
            # plus one ulp of the exponential above 1
            slack = 2.0 ** -26 / (2 * float(np.float32(sigma)) ** 2) + 2.0 ** -23
            assert abs(float(col[iy, ix]) - 1.0) <= slack and abs(float(row[iy, ix]) - 1.0) <= slack
            py, px = col[:, ix], row[iy, :]
            if sigma == 0.8:                                     # narrower, the far samples flush to 0
                assert int((py != 0).sum()) == 2 * r + 1 == int((px != 0).sum())
            want = (float(a) * py)[:, None] * px[None, :]
            normal = want.abs() >= mc.TINY32                     # below it a product may be flushed on one side and not the other
            assert want.dtype == torch.float32 and same(both[normal], want[normal]) and int(normal.sum()) >= (9 if sigma >= 0.3 else 1)
            assert bool(((both - want).abs()[~normal] <= mc.TINY32).all())
            peaks += 2
            exact += int(float(py[iy]) == 1.0) + int(float(px[ix]) == 1.0)
            # each profile against fp64, on the amplitude-1 renders themselves
            for fr, cc in ((col, (cy, np.float32(ix))), (row, (np.float32(iy), cx))):
                ref, bar = mc.bar_for(make(H, W, 1, sigma, r, [[cc]], one))
                assert mc.ratio(fr.numpy()[None], ref, bar)[0] < 1.0
        print(f"MOVIE one-hot sigma_hr {sigma}: {exact} of {peaks} peak samples are exactly 1")


def test_integer_centred_spot_is_exactly_symmetric_at_up_1():
    """up = 1, amplitude 1: a pixel is one exponential times another, so mirrored pixels hold the same number (not beyond:
    DESIGN.md 2b finding 3)"""
    for sigma in (0.8, 1.3):
        c = make(37, 70, 1, sigma, 5, [[[17.0, 40.0]]], np.ones((1, 1, 1)))
        fr = render(c)[0]
        w = fr[12:23, 35:46]
        assert float(w[5, 5]) == 1.0 and bool((w > 0).all()) and float(fr.sum()) == float(w.sum())
        assert same(w, w.flip(0)) and same(w, w.flip(1)) and same(w, w.t())


# ---- 4. the wrapper ------------------------------------------------------------------------------------------------------
def test_wrapper_handles_strides_fp64_cpu_amplitudes_and_int64_lists():
    G = gen()
    c = mc.case("lifetimes")
    want = render(c)
    args = (c["sigma"], c["H"], c["W"], c["up"], c["radius"])
    pos, amp = dev(c["pos"]), dev(c["amp"])
    fi, la = dev(c["first"]), dev(c["last"])
    keep_p, keep_a = pos.clone(), amp.clone()
    big = torch.full((c["Np"], pos.shape[1] + 3, 5), float("nan"), device="cuda")
    big[:, 2:2 + pos.shape[1], 1:3] = pos
    views = (big[:, 2:2 + pos.shape[1], 1:3], pos.transpose(0, 1).contiguous().transpose(0, 1), pos.flip(-1).flip(-1))
    assert not views[0].is_contiguous() and not views[1].is_contiguous()
    for v in views:
        assert torch.equal(v, pos) and same(G.render_movie(v, amp, *args, fi, la).cpu(), want)
    out = G.render_movie(pos.double(), amp.double(), *args, fi, la)          # fp64 holding fp32 values: the kernel reads the same
    assert out.dtype == torch.float32 and out.is_cuda and same(out.cpu(), want)
    assert same(G.render_movie(pos, torch.from_numpy(c["amp"]), *args, fi, la).cpu(), want)      # amp on the CPU
    f64, l64 = c["first"].astype(np.int64).tolist(), c["last"].astype(np.int64).tolist()
    assert same(G.render_movie(pos, amp, *args, f64, l64).cpu(), want)                            # plain lists
    assert same(G.render_movie(pos, amp, *args, torch.tensor(f64), torch.tensor(l64)).cpu(), want)
    assert torch.tensor(f64).dtype == torch.int64 and not torch.tensor(f64).is_cuda
    torch.cuda.synchronize()
    assert torch.equal(pos, keep_p) and torch.equal(amp, keep_a) and torch.equal(fi.cpu(), torch.from_numpy(c["first"]))
    assert bool(torch.isnan(big[:, :2]).all()) and bool(torch.isnan(big[..., 3:]).all())


# ---- 5. the simulator on the device ---------------------------------------------------------------------------------------
NOISE_FREE = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
LIFETIMES = [[0, 5], [2, 3], [4, 4], [1, 5]]


def simulate(seed, props=NOISE_FREE, **kw):
    out = gen().simulate_movie(4, 6, 40, 48, (0.05, 0.0004), 3, image_props=props, lifetimes=LIFETIMES, device="cuda",
                               generator=torch.Generator(device="cuda").manual_seed(seed), **kw)
    torch.cuda.synchronize()
    return out


def test_simulate_movie_on_the_device_is_seeded_and_its_truth_describes_the_movie():
    G = gen()
    movie, truth = simulate(3)
    again, truth2 = simulate(3)
    other, _ = simulate(4)
    assert movie.is_cuda and movie.dtype == torch.float32 and movie.shape == (6, 40, 48)
    assert same(movie.cpu(), again.cpu()) and not torch.equal(movie, other)
    assert set(truth) == set(truth2) and all(torch.equal(truth[k], truth2[k]) for k in truth)
    assert all(v.is_cuda for v in truth.values())
    # the structure tests/test_movie_sim.py asserts on the CPU
    assert truth["offsets"].tolist() == [0, 6, 8, 9, 14]
    assert truth["particle_id"].tolist() == [0] * 6 + [1] * 2 + [2] + [3] * 5
    assert truth["frame"].tolist() == [0, 1, 2, 3, 4, 5, 2, 3, 4, 1, 2, 3, 4, 5]
    assert truth["first"].tolist() == [0, 2, 4, 1] and truth["last"].tolist() == [5, 3, 4, 5]
    assert truth["D"].shape == (4,) and truth["D"].dtype == torch.float64 and bool((truth["D"] > 0).all())
    assert truth["pos"].shape == (4, 18, 2) and truth["pos"].dtype == torch.float32 and truth["y"].dtype == torch.float64
    assert truth["amp"].shape == (4, 6, 3) and truth["amp"].dtype == torch.float32 and "visible" not in truth
    mean_pos = truth["pos"].double().view(4, 6, 3, 2).mean(dim=2)
    assert torch.equal(truth["y"], mean_pos[truth["particle_id"], truth["frame"], 0])
    assert torch.equal(truth["x"], mean_pos[truth["particle_id"], truth["frame"], 1])
    # noise-free: the movie is the kernel's render of the truth plus the constant background, bit for bit
    sigma, up = G.psf_sigma_hr(G.DEFAULT_IMAGE_PROPS), G.DEFAULT_IMAGE_PROPS["upsampling_factor"]
    clean = G.render_movie(truth["pos"], truth["amp"], sigma, 40, 48, up, first=truth["first"], last=truth["last"])
    assert same(movie.cpu(), (clean + 20.0).cpu())
    # and within the per-pixel bar of the fp64 restatement of the truth; the sum with the background adds one rounding of
    # the sum to the rounding the bar's floor already grants
    c = make(40, 48, up, sigma, None, truth["pos"].cpu().numpy(), truth["amp"].cpu().numpy(), truth["first"].cpu().numpy(),
             truth["last"].cpu().numpy())
    ref, bar = mc.bar_for(c)
    r = mc.ratio(movie.cpu().numpy(), ref + 20.0, bar + 2 * mc.U32 * (np.abs(ref) + 20.0))
    print(f"MOVIE simulate: worst error / bar {r[0]:.3f}")
    assert r[0] < 1.0 and float(ref.max()) > 5 and float((movie[0] - 20).abs().min()) == 0


def test_simulate_movie_blink_generator_device_and_default_noise():
    G = gen()
    _, plain = simulate(3)
    dark = torch.zeros(4, 6, dtype=torch.bool)
    dark[0, 2] = dark[3, 5] = dark[1, 0] = True                  # [1, 0] lies outside particle 1's lifetime: no row for it
    movie, truth = simulate(3, blink=dark)
    assert all(v.is_cuda for v in truth.values()) and torch.equal(truth["offsets"], plain["offsets"])
    vis = truth["visible"]
    assert vis.dtype == torch.bool and vis.shape == truth["frame"].shape
    rows_dark = dark.cuda()[truth["particle_id"], truth["frame"]]
    assert torch.equal(vis, ~rows_dark) and int((~vis).sum()) == 2
    assert bool((truth["amp"][dark.cuda()] == 0).all()) and bool((truth["amp"][~dark.cuda()] != 0).all())
    assert torch.equal(truth["pos"], plain["pos"])               # a mask draws nothing: same trajectories
    lit = G.render_movie(truth["pos"], truth["amp"], G.psf_sigma_hr(G.DEFAULT_IMAGE_PROPS), 40, 48, 5, first=truth["first"],
                         last=truth["last"])
    assert same(movie.cpu(), (lit + 20.0).cpu())
    # as a probability: drawn from the generator, seeded, some rows dark and some not
    m1, t1 = simulate(5, blink=0.4)
    m2, t2 = simulate(5, blink=0.4)
    assert same(m1.cpu(), m2.cpu()) and all(torch.equal(t1[k], t2[k]) for k in t1)
    assert torch.equal(t1["offsets"], plain["offsets"]) and 0 < int((~t1["visible"]).sum()) < len(t1["visible"])
    zero = (t1["amp"] == 0).all(dim=-1)[t1["particle_id"], t1["frame"]]
    assert torch.equal(zero, ~t1["visible"])
    # a generator on the wrong device
    with pytest.raises(ValueError, match="generator"):
        G.simulate_movie(4, 6, 40, 48, 0.05, 3, device="cuda", generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="generator"):
        G.simulate_movie(4, 6, 40, 48, 0.05, 3, device="cpu", generator=torch.Generator(device="cuda").manual_seed(1))
    # the default noise: finite, seeded, and as strong as on the CPU
    a, ta = simulate(5, props=None)
    b, _ = simulate(5, props=None)
    assert a.is_cuda and bool(torch.isfinite(a).all()) and same(a.cpu(), b.cpu()) and float(a.std()) > 5
    assert ta["offsets"].tolist() == [0, 6, 8, 9, 14]
