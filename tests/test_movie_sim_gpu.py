"""GPU: the whole-field renderer mivit_render_movie (csrc/movie.hip) against the float64 restatement of the same definition
(helpers/generation.render_movie on CPU tensors), bitwise repeatability, agreement with the single-particle kernel
mivit_render_frames, and the front end (detection, linking, chaining) giving the same table on the kernel's movie as on the
restatement's.  The tolerance 2e-5 * max |ref| is the project's for this __expf arithmetic
(test_generation_gpu.py::test_render_kernel_matches_naive_loop_and_cpu_path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 37, 70                    # no multiple of the 32 x 64 tile in either direction: 2 x 2 tiles, edges at row 32, column 64
# (y, x) of the first sub-position; the others follow by a small walk
ANCHORS = [
    (10.3, 63.6),                                           # window straddles the tile edge at column 64
    (31.7, 63.9),                                           # on the corner of four tiles
    (-1.2, 20.4), (37.8, 30.1), (15.5, -0.7), (20.2, 70.6),  # partly outside, one per side
    (-30.0, 10.0), (80.0, 10.0), (10.0, -40.0), (10.0, 120.0),  # wholly outside, one per side
    (20.4, 40.2), (21.1, 41.0),                             # two particles on the same pixels
    (5.0, 5.0),                                             # gets a NaN in one sub-position
    (25.0, 50.0),                                           # every position NaN / inf
    (28.5, 8.5),                                            # exact half-pixel ties (rint to even)
]


def scene(F, npos, seed=0):
    g = torch.Generator().manual_seed(seed)
    start = torch.tensor(ANCHORS)
    Np = len(ANCHORS)
    steps = 0.3 * torch.randn(Np, F * npos, 2, generator=g)
    steps[:, 0] = 0
    pos = (start[:, None, :] + torch.cumsum(steps, dim=1)).float()
    pos[12, (F * npos) // 2, 0] = float("nan")
    pos[13, :, 0] = float("nan")
    pos[13, 0, 1] = float("inf")
    pos[14] = torch.tensor([28.5, 8.5])
    amp = (100 + 10 * torch.randn(Np, F, npos, generator=g)).float()
    return pos, amp


def check(pos, amp, sigma, up, radius, Hh=H, Ww=W, first=None, last=None, expect_empty_pixels=True):
    from moleculardiffusion_mivit_amd.helpers import generation as gen
    ref = gen.render_movie(pos, amp, sigma, Hh, Ww, up, radius, first, last)
    got = gen.render_movie(pos.cuda(), amp.cuda(), sigma, Hh, Ww, up, radius,
                           None if first is None else first.cuda(), None if last is None else last.cuda())
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == ref.shape
    got = got.cpu().double()
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"max |diff| = {err:.3e}, 2e-5 * max |ref| = {2e-5 * scale:.3e}")
    assert bool(torch.isfinite(got).all())
    assert err < 2e-5 * scale or scale == 0 and err == 0
    empty = ref == 0                                        # the restatement adds nothing outside the windows
    if expect_empty_pixels is not None:
        assert bool(empty.any()) == expect_empty_pixels
    assert bool((got[empty] == 0).all())
    return got


@pytest.mark.parametrize("F,npos,up,radius,windows", [
    (1, 1, 1, 0, False),          # a spot is its one pixel
    (3, 5, 5, None, True),        # default radius 8, first / last windows
    (1, 5, 5, 64, False),         # the radius cap: every window covers the field
    (3, 1, 5, 3, True),
    (1, 5, 1, None, False),
])
def test_kernel_matches_float64_restatement(F, npos, up, radius, windows):
    pos, amp = scene(F, npos, seed=F * 10 + npos)
    sigma = 1.3 * up
    first = last = None
    if windows:                   # visible only in frame 1; from frame 1 on; in no frame (beyond the movie, before it); always
        first = torch.tensor([1, 1, F + 1, -2] + [0] * (len(ANCHORS) - 4), dtype=torch.int32)
        last = torch.tensor([1, F - 1, F + 1, -1] + [F - 1] * (len(ANCHORS) - 4), dtype=torch.int32)
    got = check(pos, amp, sigma, up, radius, first=first, last=last, expect_empty_pixels=None if radius == 64 else True)
    if radius == 0:               # exactly one pixel per visible sub-position inside the field
        assert int((got != 0).sum()) <= len(ANCHORS) * F * npos


def test_no_particles_give_a_zero_movie():
    from moleculardiffusion_mivit_amd.helpers import generation as gen
    got = gen.render_movie(torch.zeros(0, 6, 2).cuda(), torch.zeros(0, 2, 3).cuda(), 6.5, H, W, 5)
    torch.cuda.synchronize()
    assert got.shape == (2, H, W) and bool((got == 0).all())


def test_more_particles_than_one_chunk_of_the_particle_loop():
    from moleculardiffusion_mivit_amd import ops
    Np = ops.MOVIE_PARTICLE_CHUNK + 3                       # npos 1: one pair per particle, so two passes, the second of 3
    g = torch.Generator().manual_seed(7)
    pos = (torch.rand(Np, 1, 2, generator=g) * torch.tensor([H + 6.0, W + 6.0]) - 3).float()
    amp = (100 + 10 * torch.randn(Np, 1, 1, generator=g)).float()
    check(pos, amp, 6.5, 5, 1)
    # the last particles count: without them the movie differs
    from moleculardiffusion_mivit_amd.helpers import generation as gen
    a = gen.render_movie(pos.cuda(), amp.cuda(), 6.5, H, W, 5, 1)
    b = gen.render_movie(pos[:-3].cuda(), amp[:-3].cuda(), 6.5, H, W, 5, 1)
    assert not torch.equal(a, b)


def test_two_launches_are_bitwise_equal_and_tiles_do_not_matter():
    from moleculardiffusion_mivit_amd.helpers import generation as gen
    pos, amp = scene(3, 5, seed=3)
    a = gen.render_movie(pos.cuda(), amp.cuda(), 6.5, H, W, 5)
    b = gen.render_movie(pos.cuda(), amp.cuda(), 6.5, H, W, 5)
    assert torch.equal(a, b)
    # the same scene shifted by (32, 64) pixels in a larger field falls into other tiles and other rows of a thread: same sums.
    # Positions are rounded to 2^-10 first, so that the shift is exact in fp32 (every coordinate stays below 2^8).
    q = torch.round(pos * 1024) / 1024
    base = gen.render_movie(q.cuda(), amp.cuda(), 6.5, H, W, 5)
    shifted = gen.render_movie((q + torch.tensor([32.0, 64.0])).cuda(), amp.cuda(), 6.5, H + 32, W + 64, 5)
    inner = shifted[:, 32:, 64:]
    assert torch.equal(inner, base)


@pytest.mark.parametrize("P,up", [(9, 5), (13, 3)])
def test_kernel_agrees_with_the_single_particle_kernel(P, up):
    from moleculardiffusion_mivit_amd.helpers import generation as gen
    g = torch.Generator().manual_seed(P)
    npos, F, sigma = 5, 4, 1.4 * up
    traj = (0.8 * torch.randn(1, F * npos, 2, generator=g)).clamp(-2.5, 2.5)
    amp = 100 + 10 * torch.randn(1, F, npos, generator=g)
    ref = gen.render_frames(traj.cuda(), npos, [sigma], P, up, amp.cuda(), center=False)[0, 0]
    got = gen.render_movie((traj[..., [1, 0]] + (P - 1) / 2).cuda(), amp.cuda(), sigma, P, P, up, radius=P)
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"P = {P}, up = {up}: max |diff| = {err:.3e}, 2e-5 * scale = {2e-5 * scale:.3e}")
    assert err < 2e-5 * scale


E2E_SEED = 895


def test_front_end_gives_the_same_table_on_the_kernel_movie_as_on_the_restatement():
    """24 frames of 64 x 96, five particles starting >= 20 pixels apart, D = 0.05, 5 sub-positions, constant background 20, no
    noise.  Preconditions on the restatement's movie first: it tracks perfectly, and every detected DoG peak stands more than
    1e-3 of its value (50 times the kernel's tolerance) above its eight neighbours, so no rounding difference can move a peak.
    Seed chosen with the host path of the tracker (track_particles_flat(linking="device") on the numpy movie), where both
    preconditions hold: smallest peak margin 2.85e-3."""
    from moleculardiffusion_mivit_amd.helpers import generation as gen, tracking as trk
    props = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
    ref_movie, truth = gen.simulate_movie(5, 24, 64, 96, 0.05, 5, image_props=props,
                                          generator=torch.Generator().manual_seed(E2E_SEED))
    start = truth["pos"][:, 0].double()
    assert float((torch.cdist(start, start) + 1e9 * torch.eye(5, dtype=torch.float64)).min()) >= 20
    table_ref, dog = trk.track_particles_tensors(ref_movie.cuda())
    fr, y, x, tid, long_ = (table_ref[k] for k in ("frame", "y", "x", "track_id", "in_long_track"))
    assert int(table_ref["n_tracks"]) == 5 and len(fr) == 120 and bool(long_.all())
    assert torch.bincount(tid).tolist() == [24] * 5
    s = trk.score_tracking(fr, y, x, tid, {k: v.cuda() for k, v in truth.items()})
    assert float(s["recall"]) == 1.0 and float(s["precision"]) == 1.0 and s["purity"].tolist() == [1.0] * 5
    pad = torch.nn.functional.pad(dog[None], (1, 1, 1, 1), mode="replicate")[0]
    v = dog[fr, y, x]
    around = torch.stack([pad[fr, y + 1 + dy, x + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)])
    margin = float(((v[None] - around) / v[None]).min())
    print(f"smallest relative DoG peak margin: {margin:.3e}")
    assert margin > 1e-3
    # the kernel's movie of the same scene
    up, sigma = gen.DEFAULT_IMAGE_PROPS["upsampling_factor"], gen.psf_sigma_hr(gen.DEFAULT_IMAGE_PROPS)
    hip_movie = gen.render_movie(truth["pos"].cuda(), truth["amp"].cuda(), sigma, 64, 96, up) + 20.0
    assert float((hip_movie.cpu() - ref_movie).abs().max()) < 2e-5 * float(ref_movie.abs().max())
    table_hip, _ = trk.track_particles_tensors(hip_movie)
    for k in ("frame", "y", "x", "track_id", "in_long_track"):
        assert torch.equal(table_hip[k], table_ref[k]), k
