"""GPU: the kernels of csrc/segment.hip (ops.segment_transport, ops.transport_stats) against the numpy restatements of
helpers/msd.py, which tests/test_transport.py holds against the oracle of tests/transport_common.py, and the paths that reach
them: helpers/msd.segment_transport, the raw C-ABI inside the guarded buffers of tests/abi_guard.py, and
tracking.estimate_track_diffusion(transport=...) on a simulated run-and-pause movie.

Partitions AND classes are compared EXACTLY on every track: tests/test_transport.py holds the margin of every common track
above 1e-6 in every mode, seven orders above what a 1-ulp log can move F by.  The cost is compared within
transport_common.COST_RTOL (derived there).  transport_stats has no transcendental function and is compared bit for bit."""
import numpy as np
import pytest
import torch

import transport_common as tc
from abi_call import Call, check_all
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as gen
from moleculardiffusion_mivit_amd.helpers import msd as msd_mod
from moleculardiffusion_mivit_amd.helpers import tracking as trk

pytestmark = pytest.mark.gpu

F64, I32 = torch.float64, torch.int32


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                 # a copy: the common inputs are read-only


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    """bitwise, every NaN one value (the sign of a computed NaN is the hardware's)"""
    a, b = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and bool(np.array_equal(_bits(a[~na]), _bits(b[~nb])))


def _kernel(pos, offsets, **kw):
    seg_start, seg_class, cost = ops.segment_transport(_dev(pos), _dev(np.asarray(offsets).astype(np.int32)), **kw)
    torch.cuda.synchronize()
    assert seg_start.dtype == seg_class.dtype == torch.int32 and seg_start.shape == seg_class.shape == (len(pos),)
    assert cost.dtype == torch.float64 and cost.shape == (len(offsets) - 1,)
    return seg_start.cpu().numpy(), seg_class.cpu().numpy(), cost.cpu().numpy()


def _restated(pos, offsets, mode, **kw):
    return msd_mod._transport_numpy(pos, np.asarray(offsets, np.int64), tc.MIN_LEN, tc.PENALTY, tc.VELOCITY_PENALTY, tc.MIN_VAR,
                                    tc.MODES[mode], **kw)


@pytest.fixture(scope="module")
def common():
    pos, offsets, _ = tc.common_tracks()
    want = {mode: _restated(pos, offsets, mode) for mode in tc.MODES}
    got = {mode: _kernel(pos, offsets, min_len=tc.MIN_LEN, penalty=tc.PENALTY, velocity_penalty=tc.VELOCITY_PENALTY,
                         min_var=tc.MIN_VAR, classes=mode) for mode in tc.MODES}
    return pos, offsets, want, got


@pytest.mark.parametrize("mode", sorted(tc.MODES))
def test_partition_and_classes_equal_the_restatement_on_every_track(common, mode):
    pos, offsets, want, got = common
    compared = 0
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        assert np.array_equal(got[mode][0][a:b], want[mode][0][a:b]), (k, np.nonzero(got[mode][0][a:b])[0], np.nonzero(want[mode][0][a:b])[0])
        assert np.array_equal(got[mode][1][a:b], want[mode][1][a:b]), (k, got[mode][1][a:b], want[mode][1][a:b])
        compared += 1
    assert compared == tc.N_TRACKS
    cuts, classes = tc.partition_of(got[mode][0], got[mode][1], offsets)
    if mode == "both":
        assert any(0 in c and 1 in c for c in classes)                     # both classes inside one track
    assert all(set(c) <= ({0, 1} if mode == "both" else {1} if mode == "directed" else {0}) for c in classes[1:] if c)
    want_c, got_c = want[mode][2], got[mode][2]
    assert np.array_equal(np.isnan(got_c), np.isnan(want_c)) and list(np.nonzero(np.isnan(got_c))[0]) == [0, 5]
    ok = ~np.isnan(want_c)
    err = np.abs(got_c[ok] - want_c[ok]) / (1 + np.abs(want_c[ok]))
    print(f"{mode}: worst |cost - restatement| / (1 + |cost|) = {err.max():.3g}")
    assert err.max() <= tc.COST_RTOL


def test_diffusive_mode_is_segment_tracks_bit_for_bit(common):
    pos, offsets, _, got = common
    seg_start, cost = ops.segment_tracks(_dev(pos), _dev(offsets.astype(np.int32)), min_len=tc.MIN_LEN, penalty=tc.PENALTY,
                                         min_var=tc.MIN_VAR)
    assert np.array_equal(got["diffusive"][0], seg_start.cpu().numpy()) and not got["diffusive"][1].any()
    assert _same_bits(got["diffusive"][2], cost)


def test_a_track_does_not_depend_on_its_batch(common):
    pos, offsets, _, got = common
    for k in (tc.N_TRACKS - 7, 10, 4):                                     # three planted changes; 513 rows; 9 rows
        p = pos[offsets[k]:offsets[k + 1]]
        want = tuple(g[offsets[k]:offsets[k + 1]] for g in got["both"][:2]) + (got["both"][2][k],)
        alone = _kernel(p, np.array([0, len(p)]))
        again = _kernel(p, np.array([0, len(p)]))
        other = pos[offsets[9]:offsets[10]]
        first = _kernel(np.concatenate([p, other, other]), np.array([0, len(p), len(p) + len(other), len(p) + 2 * len(other)]))
        last = _kernel(np.concatenate([other, other, p]), np.array([0, len(other), 2 * len(other), 2 * len(other) + len(p)]))
        for s, c, f in ((alone[0], alone[1], alone[2][0]), (again[0], again[1], again[2][0]),
                        (first[0][:len(p)], first[1][:len(p)], first[2][0]), (last[0][-len(p):], last[1][-len(p):], last[2][2])):
            assert np.array_equal(s, want[0]) and np.array_equal(c, want[1]), k
            assert _bits(np.array([f]))[0] == _bits(np.array([want[2]]))[0], k


def test_kernel_at_its_length_limit():
    """TRANSPORT_MAX_LEN rows: the full 147 456 B of LDS, which a workgroup gets only by asking; one row more is an error and
    no launch."""
    L = ops.TRANSPORT_MAX_LEN
    assert L == 4096
    rng = np.random.default_rng(2)
    p = np.ascontiguousarray(tc.run_and_pause(rng, 3, 2.0, (L - 1) // 4 + 1)[0][:L])
    offsets = np.array([0, L])
    want_s, want_k, want_c, margin = _restated(p, offsets, "both", return_margin=True)
    assert margin[0] >= tc.MIN_MARGIN
    got_s, got_k, got_c = _kernel(p, offsets)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_k, want_k)
    assert got_s.sum() - 1 >= 3 and 0 < got_k.sum() < L                    # the three planted cuts at least, both classes
    assert abs(got_c[0] - want_c[0]) <= tc.COST_RTOL * (1 + abs(want_c[0]))
    longer = torch.zeros(L + 1, 2, dtype=torch.float64, device="cuda")
    off = torch.tensor([0, L + 1], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=str(L)):
        ops.segment_transport(longer, off)
    with pytest.raises(ValueError, match=str(L)):
        msd_mod.segment_transport(longer, off.long())


def test_front_end_and_transport_stats_bitwise(common):
    pos, offsets, _, _ = common
    for dt, R in ((1.0, 0.0), (0.05, 1.0 / 6.0)):
        want = msd_mod.segment_transport(pos, offsets, dt=dt, blur=R)
        got = msd_mod.segment_transport(_dev(pos), _dev(offsets), dt=dt, blur=R)
        assert set(got) == set(want) and all(v.is_cuda for v in got.values())
        for k in ("seg_offsets", "seg_track", "seg_class", "n_increments", "velocity", "speed", "D_res", "D_cve", "sigma2"):
            assert got[k].dtype == torch.from_numpy(want[k]).dtype, k
            assert _same_bits(got[k], want[k]), k
        assert np.allclose(got["cost"].cpu().numpy(), want["cost"], rtol=tc.COST_RTOL, atol=tc.COST_RTOL, equal_nan=True)
    # stretches given by hand: one increment, none, two, a stretch that ends its track; rows beyond the table are never read
    seg_offsets = np.array([0, 1, 2, 4, 9, 9, 40], np.int32)
    track_end = np.array([9, 9, 9, 9, 40, 40], np.int32)
    p = pos[:40]
    got = ops.transport_stats(_dev(p), _dev(seg_offsets), _dev(track_end), 0.5, 0.1)
    want = msd_mod._transport_stats_numpy(p, seg_offsets, track_end, 0.5, 0.1)
    assert got[0].shape == (6, 2) and got[4].dtype == torch.int32
    for g, w in zip(got, want):
        assert _same_bits(g, w)
    assert got[4].tolist() == [1, 1, 2, 4, 0, 30]
    assert bool(torch.isnan(got[2][:2]).all()) and not bool(torch.isnan(got[1][:2]).any()) and bool(torch.isnan(got[0][4]).all())


ABI_LENGTHS = (5, 0, 70, 1, 9, 2)


def _abi_table(seed):
    """ABI_LENGTHS stacked; the 70-row track pauses for 35 increments and then runs at 3 step standard deviations per frame"""
    rng = np.random.default_rng(seed)
    tracks = [np.zeros((0, 2)) if L == 0 else tc.brownian(rng, L, 0.05) if L != 70 else tc.run_and_pause(rng, 1, 3.0, 35)[0][:70]
              for L in ABI_LENGTHS]
    offsets = np.concatenate([[0], np.cumsum(ABI_LENGTHS)]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(tracks, axis=0)), offsets


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("mode", sorted(tc.MODES))
def test_segment_transport_through_the_raw_abi(mode, mis):
    pos, off = _abi_table(4)
    n, n_tracks = len(pos), len(off) - 1
    want_s, want_k, want_c, margin = _restated(pos, off, mode, return_margin=True)
    assert (margin >= tc.MIN_MARGIN).all()
    if mode == "both":
        assert want_s.sum() > sum(L > 0 for L in ABI_LENGTHS) and 0 < want_k.sum(), "the planted run was not found"
    c = Call("mivit_segment_transport", mis)
    c.run(c.inp("pos", pos, F64), n, c.inp("offsets", off, I32), n_tracks, 70, tc.MIN_LEN, tc.PENALTY, tc.VELOCITY_PENALTY,
          tc.MIN_VAR, tc.MODES[mode], c.out("seg_start", n, I32), c.out("seg_class", n, I32), c.out("cost", n_tracks, F64))

    def cost_close(got, want, what):
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        ok = ~np.isnan(want)
        assert (np.abs(got[ok] - want[ok]) <= tc.COST_RTOL * (1 + np.abs(want[ok]))).all(), (what, got, want)

    check_all(c, {"seg_start": want_s, "seg_class": want_k, "cost": want_c}, close={"cost": cost_close})
    via_ops = ops.segment_transport(_dev(pos), _dev(off.astype(np.int32)), classes=mode)
    for name, t in zip(("seg_start", "seg_class", "cost"), via_ops):
        assert _same_bits(c.outs[name].numpy(), t), name


@pytest.mark.parametrize("mis", [0, 1])
def test_transport_stats_through_the_raw_abi(mis):
    rng = np.random.default_rng(6)
    rows = rng.choice([0, 1, 2, 3, 6], 257)
    rows[:3] = [3, 1, 2]
    seg_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    n, n_seg = int(seg_off[-1]), 257
    end = np.where(rng.random(n_seg) < 0.5, seg_off[1:], np.minimum(seg_off[1:] + 3, n))
    end[-1] = n
    pos = np.cumsum(rng.standard_normal((n, 2)), axis=0) + np.arange(n)[:, None] * np.array([0.4, -0.2])
    want = dict(zip(("velocity", "d_res", "d_cve", "sigma2", "n_increments"), msd_mod._transport_stats_numpy(pos, seg_off, end, 0.25, 0.1)))
    assert {0, 1, 2} <= set(want["n_increments"].tolist())
    c = Call("mivit_transport_stats", mis)
    c.run(c.inp("pos", pos, F64), n, c.inp("seg_offsets", seg_off, I32), c.inp("seg_track_end", end, I32), n_seg, 0.25, 0.1,
          c.out("velocity", (n_seg, 2), F64), c.out("d_res", n_seg, F64), c.out("d_cve", n_seg, F64), c.out("sigma2", n_seg, F64),
          c.out("n_increments", n_seg, I32))
    check_all(c, want)
    via_ops = ops.transport_stats(_dev(pos), _dev(seg_off.astype(np.int32)), _dev(end.astype(np.int32)), 0.25, 0.1)
    for name, t in zip(("velocity", "d_res", "d_cve", "sigma2", "n_increments"), via_ops):
        assert _same_bits(c.outs[name].numpy(), t), name


def test_rejected_input_raises_without_a_launch():
    pos = torch.zeros(12, 2, dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 12], dtype=torch.int32, device="cuda")
    wide = torch.zeros(12, 4, dtype=torch.float64, device="cuda")
    for bad_pos, bad_off in ((wide[:, :2], off), (pos.float(), off), (pos, off.long()), (pos.cpu(), off), (pos[:, :1], off),
                             (pos, torch.tensor([0, 11], dtype=torch.int32, device="cuda")),
                             (pos, torch.arange(0, 26, 2, dtype=torch.int32, device="cuda")[::2])):
        with pytest.raises(ValueError):
            ops.segment_transport(bad_pos, bad_off)
    for kw in ({"min_len": 1}, {"penalty": -1.0}, {"velocity_penalty": -1.0}, {"min_var": 0.0}, {"min_var": float("inf")},
               {"classes": "runs"}, {"classes": 0}):
        with pytest.raises(ValueError):
            ops.segment_transport(pos, off, **kw)
        with pytest.raises(ValueError):
            msd_mod.segment_transport(pos, off.long(), **kw)
    for kw in ({"dt": 0.0}, {"blur": 0.3}):
        with pytest.raises(ValueError):
            msd_mod.segment_transport(pos, off.long(), **kw)
    end = torch.tensor([12], dtype=torch.int32, device="cuda")
    for args in ((wide[:, :2], off, end), (pos.float(), off, end), (pos, off, end.long()), (pos, off, off)):
        with pytest.raises(ValueError):
            ops.transport_stats(*args)
    for kw in ({"dt": 0.0}, {"blur": -0.1}):
        with pytest.raises(ValueError):
            ops.transport_stats(pos, off, end, **kw)
    # the entry itself refuses what ops refuses: an error string, no launch
    from moleculardiffusion_mivit_amd import _native as N
    out_i, out_k = torch.zeros(12, dtype=torch.int32, device="cuda"), torch.zeros(12, dtype=torch.int32, device="cuda")
    cost = torch.zeros(1, dtype=torch.float64, device="cuda")
    for max_len, min_len, pen, vpen, mv, cls in ((4097, 4, 3.0, 3.0, 1e-12, 0), (12, 1, 3.0, 3.0, 1e-12, 0), (12, 4, -1.0, 3.0, 1e-12, 0),
                                                 (12, 4, 3.0, -1.0, 1e-12, 0), (12, 4, 3.0, 3.0, 0.0, 0), (12, 4, 3.0, 3.0, 1e-12, 3)):
        rc = N.lib.mivit_segment_transport(pos.data_ptr(), 12, off.data_ptr(), 1, max_len, min_len, pen, vpen, mv, cls,
                                           out_i.data_ptr(), out_k.data_ptr(), cost.data_ptr(), None)
        assert rc != 0 and b"segment_transport" in N.lib.mivit_last_error()
    torch.cuda.synchronize()
    assert not out_i.any() and not out_k.any() and not cost.any()


class MeanPixel(torch.nn.Module):
    def forward(self, seq):
        return seq.mean(dim=(1, 2, 3)).unsqueeze(1)


E2E_SEED = 14                                                          # see the docstring below


def test_end_to_end_on_a_run_and_pause_movie():
    """6 particles, 80 frames of 96 x 96, noise-free, D = 0.05 in both states, state velocities ((0, 0), (0, 0.6)): every
    particle pauses for 40 frames and runs for 40, or the reverse (the path is planted, M is the identity).  A matched track is
    one that score_tracking gives to one particle with purity 1 and that has at least 2 * min_len + 5 = 13 rows on either side
    of frame 40.  Each must have exactly one cut, within 5 frames of frame 40, the run in class 1 and the pause in class 0, and
    the run's velocity_ml within 4 velocity_ml_std of (0, 0.6).  The seed was picked among 11 .. 16 as one whose movie meets
    this on every one of its 6 tracks (measured: cuts at frames 38 .. 41, run velocities (-0.09 .. 0.02, 0.51 .. 0.58) +- 0.04);
    12, 13 and 15 do as well, on 5, 2 and 5 matched tracks; 11 has one track of four whose cut lies at frame 30, and 16 one
    with a spurious run of 4 frames at its start: what the statistics of DESIGN 4v lead one to expect of two dozen tracks."""
    Np, F_ = 6, 80
    path = torch.from_numpy(tc.planted_path(Np, F_, 40))
    V = torch.tensor([[0.0, 0.0], [0.0, 0.6]], dtype=torch.float64)
    props = {"background_intensity": [20.0, 0.0], "poisson_noise": -1}
    g = torch.Generator(device="cuda").manual_seed(E2E_SEED)
    movie, truth = gen.simulate_movie(Np, F_, 96, 96, None, 2, image_props=props, generator=g, device="cuda",
                                      states={"Ds": (0.05, 0.05), "M": np.eye(2), "path": path, "velocity": V})
    assert torch.equal(truth["state"].view(Np, F_).cpu(), path)
    assert torch.equal(truth["velocity_row"], V.cuda()[truth["state"]])
    model = MeanPixel().cuda()
    base = trk.estimate_track_diffusion(movie, model, 10, max_gap=2, directed={})
    res = trk.estimate_track_diffusion(movie, model, 10, max_gap=2, directed={}, transport={})
    assert set(res) == set(base) | {"transport", "run_fraction", "n_runs"}
    for k in base:                                                         # the entries that exist today, bit for bit
        if isinstance(base[k], dict):
            assert set(base[k]) == set(res[k]) and all(_same_bits(base[k][j], res[k][j]) for j in base[k] if torch.is_tensor(base[k][j])), k
        else:
            assert _same_bits(base[k], res[k]), k
    tr = res["transport"]
    n_seg, n_tracks = len(tr["seg_track"]), len(res["track_id"])
    assert set(tr) == {"seg_offsets", "seg_track", "seg_class", "velocity", "speed", "D_res", "D_cve", "sigma2", "n_increments", "cost",
                       "D_model", "n_sequences", "velocity_ml", "velocity_ml_std", "speed_ml", "D_dir", "D_dir_std", "lr_directed",
                       "p_directed", "directed_status"}
    assert tr["seg_offsets"].shape == (n_seg + 1,) and tr["cost"].shape == (n_tracks,)
    assert tr["velocity"].shape == tr["velocity_ml"].shape == tr["velocity_ml_std"].shape == (n_seg, 2)
    for k in ("seg_class", "speed", "D_res", "D_cve", "sigma2", "n_increments", "D_model", "n_sequences", "speed_ml", "D_dir", "D_dir_std",
              "lr_directed", "p_directed", "directed_status"):
        assert tr[k].shape == (n_seg,), k
    seg_len = tr["seg_offsets"][1:] - tr["seg_offsets"][:-1]
    assert torch.equal(tr["n_sequences"], seg_len // 10)
    assert res["run_fraction"].shape == res["n_runs"].shape == (n_tracks,)
    assert bool(((res["run_fraction"] >= 0) & (res["run_fraction"] <= 1)).all())
    with_ml = trk.estimate_track_diffusion(movie, model, 10, max_gap=2, ml={}, transport={"classes": "both"})
    assert {"D_ml", "D_ml_std", "ml_status"} <= set(with_ml["transport"]) and with_ml["transport"]["D_ml"].shape == (n_seg,)
    assert "velocity_ml" not in with_ml["transport"] and _same_bits(with_ml["transport"]["seg_offsets"], tr["seg_offsets"])
    # the cuts, classes and velocities of the matched tracks
    table, _ = trk.track_particles_tensors(movie, return_dog=False, max_gap=2)
    fr, y, x, tid, offsets = trk.tracks_table_by_track(table)[:5]
    score = trk.score_tracking(fr, y, x, tid, truth)
    assert torch.equal(score["track_id"], res["track_id"])
    fr, offsets = fr.cpu().numpy(), offsets.cpu().numpy()
    so, st, cls = tr["seg_offsets"].cpu().numpy(), tr["seg_track"].cpu().numpy(), tr["seg_class"].cpu().numpy()
    vml, vsd = tr["velocity_ml"].cpu().numpy(), tr["velocity_ml_std"].cpu().numpy()
    need = 2 * 4 + 5
    checked = 0
    for k in range(n_tracks):
        f = fr[offsets[k]:offsets[k + 1]]
        pid = int(score["particle_id"][k])
        if pid < 0 or float(score["purity"][k]) < 1.0 or f[0] > 40 - need or f[-1] < 40 + need:
            continue
        rows = np.nonzero(st == k)[0]
        cut_frames = fr[so[:-1][rows[1:]]]
        print(f"track {k}: particle {pid}, frames {f[0]} .. {f[-1]}, cuts at frames {cut_frames}, classes {cls[rows]}, "
              f"velocity_ml {vml[rows].round(3).tolist()} +- {vsd[rows].round(3).tolist()}")
        assert len(cut_frames) == 1 and abs(int(cut_frames[0]) - 40) <= 5, (k, cut_frames)
        want_cls = [0, 1] if pid % 2 == 0 else [1, 0]                      # even particles pause first
        assert cls[rows].tolist() == want_cls, (k, cls[rows])
        run = rows[want_cls.index(1)]
        assert (np.abs(vml[run] - np.array([0.0, 0.6])) <= 4 * vsd[run]).all(), (k, vml[run], vsd[run])
        assert float(res["n_runs"][k]) == 1 and 0 < float(res["run_fraction"][k]) < 1
        checked += 1
    print(f"{checked} of {n_tracks} tracks checked")
    assert checked >= 1                                                    # not vacuous
