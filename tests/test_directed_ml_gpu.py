"""GPU: the kernels of csrc/directed_ml.hip through the raw C-ABI inside the guarded, poisoned buffers of tests/abi_guard.py
and through ops, on the 74 ranges of tests/directed_ml_common.batch: mivit_track_directed_ml against the numpy restatement
(helpers/msd._directed_ml_numpy), which tests/test_directed_ml.py holds against the dense likelihood, a polish and tracks
drawn from outside the model; mivit_track_directed_loglik against the restatement with the velocity given and profiled; null
arguments; that a range's outputs are bitwise the same alone, in the batch and in every launch; hostile offsets; the empty
problems and the error codes; and the path that reaches the kernel from a movie,
tracking.estimate_track_diffusion(directed=...).  The bars are in directed_ml_common.BARS, with their origin."""
import ctypes
from functools import lru_cache, partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import directed_ml_common as dc
from abi_call import Call, bits_equal, check_all, same_results
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as G
from moleculardiffusion_mivit_amd.helpers import models as MD
from moleculardiffusion_mivit_amd.helpers import msd as M
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

F64, I32, U8 = torch.float64, torch.int32, torch.uint8
OUTS = ("D", "D_std", "velocity", "velocity_std", "loglik", "n_increments", "status")       # the order of the C-ABI
LOGLIK_AT_BAR = 1e-10         # mivit_track_directed_loglik against the restatement at the same parameters, relative


def shape_of(k, n):
    return (n, 2) if k.startswith("velocity") else n


def type_of(k):
    return I32 if k in ("n_increments", "status") else F64


@lru_cache(maxsize=None)
def the_batch():
    return dc.batch()


def args_of(b, var=True, frames=True, use=True):
    return (b["pos"], b["var"] if var else None, b["frames"].astype(np.int64) if frames else None, b["use"] if use else None,
            b["offsets"], dc.BATCH_DT, dc.BATCH_R)


@lru_cache(maxsize=None)
def restatement():
    """computed once on the CPU; the tests read it and leave it as it is"""
    want = dict(zip(OUTS, M._directed_ml_numpy(*args_of(the_batch()))))
    assert (want["status"] == 0).sum() >= dc.MIN_STATUS_0
    return want


def inputs(c, b, raw_offsets=None, var=True, frames=True, use=True):
    raw = b["offsets"] if raw_offsets is None else raw_offsets
    return (c.inp("pos", b["pos"], F64), c.inp("var", b["var"], F64) if var else None,
            c.inp("frames", b["frames"], I32) if frames else None, c.inp("use", b["use"].astype(np.uint8), U8) if use else None,
            len(b["pos"]), c.inp("offsets", raw, I32), len(raw) - 1, dc.BATCH_DT, dc.BATCH_R)


def ml_call(b, mis=0, **kw):
    c = Call("mivit_track_directed_ml", mis)
    n = len(b["offsets"]) - 1
    c.run(*inputs(c, b, **kw), *(c.out(k, shape_of(k, n), type_of(k)) for k in OUTS))
    return c


def loglik_call(b, mis=0, given=True, **kw):
    c = Call("mivit_track_directed_loglik", mis)
    n = len(b["offsets"]) - 1
    c.run(*inputs(c, b, **kw), c.inp("D", b["D"], F64), c.inp("v", b["velocity"], F64) if given else None, c.out("loglik", n, F64),
          None if given else c.out("velocity", (n, 2), F64), None if given else c.out("velocity_std", (n, 2), F64))
    return c


def compare(got, want, names):
    """the outputs of the kernel (dict of arrays) against the restatement's, by the bars of directed_ml_common.BARS"""
    assert np.array_equal(got["status"], want["status"]), [(names[k], int(got["status"][k]), int(want["status"][k]))
                                                             for k in np.nonzero(got["status"] != want["status"])[0]]
    assert np.array_equal(got["n_increments"], want["n_increments"])
    for k in OUTS[:5]:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        inf = np.isinf(want[k])
        assert np.array_equal(np.isinf(got[k]), inf) and np.array_equal(got[k][inf], want[k][inf]), k
    for k in ("D", "D_std", "loglik"):
        ok = np.isfinite(want[k]) & (want[k] != 0)
        assert np.array_equal(got[k][~ok & ~np.isnan(want[k])], want[k][~ok & ~np.isnan(want[k])]), k      # D = 0 at status 2
        rel = np.abs(got[k][ok] - want[k][ok]) / np.abs(want[k][ok])
        print(f"{k}: worst relative difference {rel.max():.3g} (bar {dc.BARS[k]:g})")
        assert (rel <= dc.BARS[k]).all(), (k, [names[i] for i in np.nonzero(ok)[0][rel > dc.BARS[k]]])
    ok = np.isfinite(want["velocity"]).all(axis=1)
    err = np.abs(got["velocity"][ok] - want["velocity"][ok]) / want["velocity_std"][ok]
    print(f"velocity: worst difference in units of its standard error {err.max():.3g} (bar {dc.BARS['velocity']:g})")
    assert (err <= dc.BARS["velocity"]).all(), [names[i] for i in np.nonzero(ok)[0][(err > dc.BARS["velocity"]).any(axis=1)]]
    rel = np.abs(got["velocity_std"][ok] / want["velocity_std"][ok] - 1.0)
    print(f"velocity_std: worst relative difference {rel.max():.3g} (bar {dc.BARS['velocity_std']:g})")
    assert (rel <= dc.BARS["velocity_std"]).all()


def test_the_batch_holds_its_ranges():
    b, want = the_batch(), restatement()
    assert len(b["names"]) == 74 and int(np.diff(b["offsets"]).max()) == 300
    assert set(want["status"].tolist()) >= {0, 1, 2}
    inc = dict(zip(b["names"], want["n_increments"].tolist()))
    st = dict(zip(b["names"], want["status"].tolist()))
    k = {name: i for i, name in enumerate(b["names"])}
    assert inc["3 rows, directed"] == 2 and st["3 rows, directed"] != 1 and inc["300 rows, directed"] == 299
    line = k["straight line, no variance"]
    assert st["straight line, no variance"] == 2 and want["loglik"][line] == -np.inf and np.isnan(want["velocity"][line]).all()
    noisy = k["straight line within its noise"]
    assert st["straight line within its noise"] == 2 and np.isfinite(want["velocity"][noisy]).all() and want["D"][noisy] == 0.0
    assert (np.abs(want["velocity"][noisy] - dc.LINE_VELOCITY) < 3.0 * want["velocity_std"][noisy]).all()
    fast = k["fast"]
    assert st["fast"] == 0 and (np.abs(want["velocity"][fast] - b["velocity"][fast]) < 4.0 * want["velocity_std"][fast]).all()
    assert np.hypot(*b["velocity"][fast]) * dc.BATCH_DT == pytest.approx(dc.FAST * np.sqrt(2.0 * 0.05 * dc.BATCH_DT))


@pytest.mark.parametrize("mis", [0, 1])
def test_fit_through_the_raw_abi_against_the_restatement(mis):
    c = ml_call(the_batch(), mis)
    want = restatement()
    check_all(c, {"status": want["status"], "n_increments": want["n_increments"]})      # every entry written, no poison left
    for k in OUTS[:5]:
        assert not c.outs[k].unchanged().numpy().any(), k
    compare({k: c.outs[k].numpy() for k in OUTS}, want, the_batch()["names"])


def test_fit_through_ops_against_the_restatement():
    b = the_batch()
    n = len(b["names"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("pos", "var", "frames", "use", "offsets", "D", "velocity")}
    got = ops.track_directed_ml(dev["pos"], dev["offsets"].int(), dev["var"], dev["frames"], dev["use"], dt=dc.BATCH_DT, blur=dc.BATCH_R)
    assert [g.dtype for g in got] == [F64] * 5 + [I32, I32] and got[2].shape == got[3].shape == (n, 2)
    compare({k: g.cpu().numpy() for k, g in zip(OUTS, got)}, restatement(), b["names"])
    raw = ml_call(b)
    for k, g in zip(OUTS, got):
        assert g.is_cuda and bits_equal(g.cpu().numpy(), raw.outs[k].numpy()), k
    # the front ends on CUDA tensors are these calls
    fit = M.estimate_directed_ml(dev["pos"], dev["offsets"], dev["var"], frames=dev["frames"], use=dev["use"], dt=dc.BATCH_DT, blur=dc.BATCH_R)
    for k, g in zip(M._DM_OUTS, got):
        assert fit[k].is_cuda and bits_equal(fit[k].double().cpu().numpy(), g.double().cpu().numpy()), k
    assert fit["status"].dtype == fit["n_increments"].dtype == torch.int64
    free = M.estimate_diffusion_ml(dev["pos"], dev["offsets"], dev["var"], frames=dev["frames"], use=dev["use"], dt=dc.BATCH_DT, blur=dc.BATCH_R)
    assert bits_equal(fit["lr_brownian"].cpu().numpy(), (2.0 * (got[4] - free["loglik"])).cpu().numpy())
    fine = ((fit["status"] == 0) & (free["status"] == 0)).cpu().numpy()
    lr, p = fit["lr_brownian"].cpu().numpy(), fit["p_brownian"].cpu().numpy()
    assert (lr[fine] >= -1e-6).all(), lr[fine].min()
    assert np.array_equal(np.isnan(p), np.isnan(lr))                       # the device's exp is not the host's to the last bit
    assert np.allclose(p[~np.isnan(p)], np.exp(-0.5 * np.maximum(lr[~np.isnan(p)], 0.0)), rtol=1e-13, atol=0.0)
    host = M.estimate_directed_ml(b["pos"], b["offsets"], b["var"], b["frames"].astype(np.int64), b["use"], dc.BATCH_DT, dc.BATCH_R)
    ok = np.isfinite(host["speed"])
    assert np.array_equal(np.isnan(fit["speed"].cpu().numpy()), np.isnan(host["speed"]))
    assert np.allclose(fit["speed"].cpu().numpy()[ok], host["speed"][ok], rtol=1e-5, atol=0)
    ll = M.directed_loglik(dev["pos"], dev["offsets"], dev["D"], dev["velocity"], dev["var"], frames=dev["frames"], use=dev["use"],
                           dt=dc.BATCH_DT, blur=dc.BATCH_R)
    assert set(ll) == {"loglik"} and ll["loglik"].is_cuda and bits_equal(ll["loglik"].cpu().numpy(), loglik_call(b).outs["loglik"].numpy())
    prof = M.directed_loglik(dev["pos"], dev["offsets"], dev["D"], None, dev["var"], frames=dev["frames"], use=dev["use"],
                             dt=dc.BATCH_DT, blur=dc.BATCH_R)
    raw = loglik_call(b, given=False)
    for k in ("loglik", "velocity", "velocity_std"):
        assert prof[k].is_cuda and bits_equal(prof[k].cpu().numpy(), raw.outs[k].numpy()), k
    with pytest.raises(ValueError, match="dt"):
        ops.track_directed_ml(dev["pos"], dev["offsets"].int(), dt=0.0)
    with pytest.raises(ValueError, match="blur"):
        ops.track_directed_ml(dev["pos"], dev["offsets"].int(), blur=0.3)
    with pytest.raises(ValueError, match="blur"):
        ops.track_directed_loglik(dev["pos"], dev["offsets"].int(), dev["D"], blur=-0.1)
    with pytest.raises(ValueError, match="offsets"):
        ops.track_directed_ml(dev["pos"], dev["offsets"].int()[:-1], dev["var"])
    with pytest.raises(ValueError, match="var"):
        ops.track_directed_ml(dev["pos"], dev["offsets"].int(), dev["var"][:-1])
    with pytest.raises(ValueError, match="D must"):
        ops.track_directed_loglik(dev["pos"], dev["offsets"].int(), dev["D"][:-1])
    with pytest.raises(ValueError, match="velocity"):
        ops.track_directed_loglik(dev["pos"], dev["offsets"].int(), dev["D"], dev["velocity"][:-1])


@pytest.mark.parametrize("given", [True, False])
def test_loglik_against_the_restatement(given):
    b = the_batch()
    n = len(b["names"])
    c = loglik_call(b, mis=0 if given else 1, given=given)
    got = c.outs["loglik"].numpy()
    assert all(not o.unchanged().numpy().any() for o in c.outs.values())
    want, wv, ws = M._directed_loglik_numpy(*args_of(b), b["D"], b["velocity"] if given else None)
    # 0 rows, 1 row, every row unusable, one usable row
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 4 and np.isfinite(want).sum() >= 65
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    ok = np.isfinite(want)
    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
    print(f"velocity given {given}: worst relative difference of loglik to the restatement {rel.max():.3g} (bar {LOGLIK_AT_BAR:g})")
    assert (rel <= LOGLIK_AT_BAR).all()
    if not given:                                                          # the same D on both sides: the arithmetic alone differs
        gv, gs = c.outs["velocity"].numpy(), c.outs["velocity_std"].numpy()
        assert np.array_equal(np.isnan(gv), np.isnan(wv)) and np.array_equal(np.isnan(gs), np.isnan(ws))
        okv = np.isfinite(wv).all(axis=1)
        err = max(float((np.abs(gv - wv)[okv] / ws[okv]).max()), float(np.abs(gs[okv] / ws[okv] - 1.0).max()))
        print(f"profiled velocity and its standard error: worst difference {err:.3g} (bar {dc.BARS['velocity']:g})")
        assert err <= dc.BARS["velocity"]
    # D negative or not finite: NaN
    odd = np.arange(n) % 2 == 0
    bad = dict(b, D=np.where(odd, np.where(np.arange(n) % 4 == 0, -1.0, np.inf), b["D"]))
    out = loglik_call(bad, given=given)
    for k, o in out.outs.items():
        assert np.isnan(o.numpy()[odd]).all() and bits_equal(o.numpy()[~odd], c.outs[k].numpy()[~odd]), k


@pytest.mark.parametrize("var,frames,use", [(False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_null_arguments_are_the_defaults(var, frames, use):
    b = dict(the_batch())
    if not use:                                                            # without flags every row counts: keep them finite
        b["pos"] = np.where(np.isfinite(b["pos"]), b["pos"], 1.0)
        b["var"] = np.where(np.isfinite(b["var"]) & (b["var"] >= 0), b["var"], 0.01)
    n = len(b["pos"])
    full = dict(b, var=b["var"] if var else np.zeros((n, 2)), use=b["use"] if use else np.ones(n, bool),
                frames=b["frames"] if frames else np.concatenate([np.arange(e - a) for a, e in zip(b["offsets"][:-1], b["offsets"][1:])]))
    same_results(ml_call(b, var=var, frames=frames, use=use), ml_call(full))
    same_results(loglik_call(b, var=var, frames=frames, use=use), loglik_call(full))
    same_results(loglik_call(b, given=False, var=var, frames=frames, use=use), loglik_call(full, given=False))


def test_a_range_alone_is_the_range_in_the_batch():
    """n = 1 with the offsets of each range in turn, on the same device buffers: bitwise the batch's entry; and the batch twice"""
    b = the_batch()
    n = len(b["names"])
    first, second = ml_call(b), ml_call(b)
    same_results(first, second)
    ll_first, ll_second = loglik_call(b, given=False), loglik_call(b, given=False)
    same_results(ll_first, ll_second)
    dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("pos", "var", "frames", "D")}
    dev["use"] = torch.from_numpy(b["use"].astype(np.uint8)).cuda()
    off = torch.from_numpy(b["offsets"].astype(np.int32)).cuda()
    outs = {k: torch.zeros(shape_of(k, n), dtype=type_of(k), device="cuda") for k in OUTS}
    ll = {k: torch.zeros(shape_of(k, n), dtype=F64, device="cuda") for k in ("loglik", "velocity", "velocity_std")}
    p = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = (p(dev["pos"]), p(dev["var"]), p(dev["frames"]), p(dev["use"]), len(b["pos"]))
    for k in range(n):
        N.check(N.lib.mivit_track_directed_ml(*rows, p(off[k:k + 2]), 1, dc.BATCH_DT, dc.BATCH_R, *(p(outs[o][k:k + 1]) for o in OUTS), stream),
                "mivit_track_directed_ml")
        N.check(N.lib.mivit_track_directed_loglik(*rows, p(off[k:k + 2]), 1, dc.BATCH_DT, dc.BATCH_R, p(dev["D"][k:k + 1]), None,
                                                  p(ll["loglik"][k:k + 1]), p(ll["velocity"][k:k + 1]), p(ll["velocity_std"][k:k + 1]), stream),
                "mivit_track_directed_loglik")
    torch.cuda.synchronize()
    for o in OUTS:
        assert bits_equal(outs[o].cpu().numpy(), first.outs[o].numpy()), o
    for o in ll:
        assert bits_equal(ll[o].cpu().numpy(), ll_first.outs[o].numpy()), o


def test_hostile_offsets_are_clamped():
    """the first offset below 0 and the last above N: the ranges keep their rows, nothing outside [0, N) is read"""
    import abi_guard as guard
    b = the_batch()
    raw = np.array(b["offsets"], np.int64)
    raw[0], raw[-1] = -3, len(b["pos"]) + 2
    hostile = guard.bounded(raw, 0, len(b["pos"]), 16)
    same_results(ml_call(b, raw_offsets=hostile), ml_call(b))
    same_results(loglik_call(b, raw_offsets=hostile), loglik_call(b))
    same_results(loglik_call(b, given=False, raw_offsets=hostile), loglik_call(b, given=False))


def test_empty_problems_and_error_codes():
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = [None] * 4
    assert N.lib.mivit_track_directed_ml(*none, 0, None, 0, 1.0, 0.0, *[None] * 7, stream) == 0
    assert N.lib.mivit_track_directed_loglik(*none, 0, None, 0, 1.0, 0.0, *[None] * 5, stream) == 0
    c = Call("mivit_track_directed_ml")                                    # no rows, two ranges: both are empty
    c.run(*none, 0, c.inp("offsets", np.zeros(3, np.int64), I32), 2, 1.0, 0.0, *(c.out(k, shape_of(k, 2), type_of(k)) for k in OUTS))
    check_all(c, dict({k: np.full(shape_of(k, 2), np.nan) for k in OUTS[:5]}, n_increments=np.zeros(2), status=np.ones(2)))
    c = Call("mivit_track_directed_loglik")
    c.run(*none, 0, c.inp("offsets", np.zeros(3, np.int64), I32), 2, 1.0, 0.0, c.inp("D", np.ones(2), F64), None,
          c.out("loglik", 2, F64), c.out("velocity", (2, 2), F64), c.out("velocity_std", (2, 2), F64))
    check_all(c, {"loglik": np.full(2, np.nan), "velocity": np.full((2, 2), np.nan), "velocity_std": np.full((2, 2), np.nan)})
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        assert N.lib.mivit_track_directed_ml(*none, 0, None, 0, dt, 0.0, *[None] * 7, stream) != 0
        assert N.lib.mivit_track_directed_loglik(*none, 0, None, 0, dt, 0.0, *[None] * 5, stream) != 0
    for blur in (-0.01, 0.26, float("nan")):
        assert N.lib.mivit_track_directed_ml(*none, 0, None, 0, 1.0, blur, *[None] * 7, stream) != 0
        assert N.lib.mivit_track_directed_loglik(*none, 0, None, 0, 1.0, blur, *[None] * 5, stream) != 0
    assert N.lib.mivit_track_directed_ml(*none, -1, None, 0, 1.0, 0.0, *[None] * 7, stream) != 0
    off = torch.zeros(2, dtype=I32, device="cuda")
    po = ctypes.c_void_p(off.data_ptr())
    assert N.lib.mivit_track_directed_ml(*none, 0, po, 1, 1.0, 0.0, *[None] * 7, stream) != 0, "null outputs"
    assert N.lib.mivit_track_directed_ml(*none, 5, po, 1, 1.0, 0.0, *[po] * 7, stream) != 0, "null pos"
    assert N.lib.mivit_track_directed_loglik(*none, 0, po, 1, 1.0, 0.0, None, None, po, None, None, stream) != 0, "null D"
    assert N.lib.mivit_track_directed_loglik(*none, 0, po, 1, 1.0, 0.0, po, None, None, None, None, stream) != 0, "null loglik"
    empty = (torch.zeros(0, 2, dtype=F64, device="cuda"), torch.zeros(1, dtype=I32, device="cuda"))
    assert all(len(g) == 0 for g in ops.track_directed_ml(*empty))
    assert all(len(g) == 0 for g in ops.track_directed_loglik(*empty, torch.zeros(0, dtype=F64, device="cuda")))


# ----------------------------------------------------------------------------------------------------------------------
# estimate_track_diffusion(directed=)
# ----------------------------------------------------------------------------------------------------------------------
SEQ_LEN, PATCH, BATCH, DT = 5, 9, 16, 0.03
CAMERA = {"background": 10.0, "gain": 2.0, "offset": 100.0, "read_noise": 2.0}
NEW = {"velocity_ml", "velocity_ml_std", "speed_ml", "speed_ml_std", "D_dir", "D_dir_std", "lr_directed", "p_directed",
       "directed_status", "directed"}


def _bits(a, b):
    return a.dtype == b.dtype and bits_equal(a.double().cpu().numpy(), b.double().cpu().numpy())


def test_estimate_track_diffusion_with_directed():
    """a 3-particle, 12-frame, 64 x 64 camera movie whose particles each move at a velocity of their own; with this seed they
    stay 16 pixels apart and 12 pixels inside the field"""
    vel = np.array([[0.8, 0.4], [-0.6, 0.7], [0.3, -0.8]])
    movie, truth = G.simulate_movie(3, 12, 64, 64, 0.2, 4, image_props={"particle_intensity": [300.0, 5.0]}, camera=CAMERA,
                                    generator=torch.Generator().manual_seed(29), margin=10.0, velocity=vel)
    dm = movie.cuda()
    props = dict(G.DEFAULT_IMAGE_PROPS)
    loc = {"gain": CAMERA["gain"], "offset": CAMERA["offset"], "read_var": (CAMERA["read_noise"] / CAMERA["gain"]) ** 2,
           "sigma0": G.psf_sigma_hr(props) / props["upsampling_factor"]}
    torch.manual_seed(0)
    model = MD.GeneralTransformer(MD.LinearProjectionEmbedding, dict(patch_size=PATCH, embed_dim=64), 64, 4, 128, 1,
                                  partial(MD.MLPHead, hidden_dim=128, output_dim=1), F.relu, precision="fp32").cuda()
    kw = dict(patch_size=PATCH, dt=DT, batch_size=BATCH, min_track_length=5, max_gap=2, localization=loc)
    base = T.estimate_track_diffusion(dm, model, SEQ_LEN, **kw)
    none = T.estimate_track_diffusion(dm, model, SEQ_LEN, directed=None, **kw)
    res = T.estimate_track_diffusion(dm, model, SEQ_LEN, directed={"blur": dc.R_FRAME}, **kw)

    def same(a, b, extra=frozenset()):
        assert set(a) == set(b) | extra
        for k, v in b.items():
            if isinstance(v, dict):
                same(a[k], v)
            elif torch.is_tensor(v):
                assert _bits(a[k], v), k
            elif isinstance(v, np.ndarray):
                assert bits_equal(a[k], v), k
            else:
                assert a[k] == v or (a[k] != a[k] and v != v), k

    same(none, base)                                                       # directed=None: exactly today's keys and bits
    same(res, base, NEW)                                                   # ... and directed adds to them, changing none
    n_tracks = len(res["track_id"])
    assert n_tracks >= 2 and res["velocity_ml"].shape == res["velocity_ml_std"].shape == (n_tracks, 2)
    assert all(res[k].shape == (n_tracks,) for k in NEW - {"directed", "velocity_ml", "velocity_ml_std"})
    assert res["directed_status"].dtype == torch.int64
    table, _ = T.track_particles_tensors(dm, return_dog=False, min_track_length=5, max_gap=2)
    fr, y, x, tid, offsets, filled = T.tracks_table_by_track(table)
    fit = T.refine_localizations_tensors(T.extract_patches_flat(dm.float(), fr, y, x, PATCH), y, x, method="mle", camera=loc)
    dm_args = res["directed"]
    assert set(dm_args) == {"positions", "variances", "frames", "use", "blur"} and dm_args["blur"] == dc.R_FRAME
    assert _bits(dm_args["positions"], torch.stack([fit["y_refined"], fit["x_refined"]], dim=1))
    assert _bits(dm_args["variances"], torch.stack([fit["y_std"] ** 2, fit["x_std"] ** 2], dim=1))
    assert torch.equal(dm_args["frames"], fr) and torch.equal(dm_args["use"], (fit["status"] == 0) & ~filled)
    columns = (("velocity_ml", "velocity"), ("velocity_ml_std", "velocity_std"), ("speed_ml", "speed"), ("speed_ml_std", "speed_std"),
               ("D_dir", "D_dir"), ("D_dir_std", "D_dir_std"), ("lr_directed", "lr_brownian"), ("p_directed", "p_brownian"),
               ("directed_status", "status"))
    want = M.estimate_directed_ml(dm_args["positions"], offsets, dm_args["variances"], frames=fr, use=dm_args["use"], dt=DT, blur=dc.R_FRAME)
    for k, key in columns:
        assert _bits(res[k], want[key]), k
    # the same rows on the host (the numpy restatement), within the bars of the kernel tests
    host = M.estimate_directed_ml(dm_args["positions"].cpu(), offsets.cpu(), dm_args["variances"].cpu(), frames=fr.cpu(),
                                  use=dm_args["use"].cpu(), dt=DT, blur=dc.R_FRAME)
    got = {key: res[k].cpu().numpy() for k, key in columns}
    host = {k: v.numpy() for k, v in host.items()}
    print("status", got["status"].tolist(), "velocity_ml (pixels per frame)", (got["velocity"] * DT).round(3).tolist(), "truth", vel.tolist(),
          "lr_directed", got["lr_brownian"].round(2).tolist())
    assert np.array_equal(got["status"], host["status"]) and (got["status"] == 0).sum() >= 2
    fine = host["status"] == 0
    for k, bar in (("D_dir", dc.BARS["D"]), ("D_dir_std", dc.BARS["D_std"]), ("velocity_std", dc.BARS["velocity_std"]),
                   ("speed", dc.BARS["velocity"]), ("speed_std", dc.BARS["velocity_std"])):
        scale = host["speed_std"][fine] if k == "speed" else np.abs(host[k][fine])
        assert (np.abs(got[k][fine] - host[k][fine]) / scale <= bar).all(), k
    assert (np.abs(got["velocity"][fine] - host["velocity"][fine]) / host["velocity_std"][fine] <= dc.BARS["velocity"]).all()
    # lr is a difference of two log-likelihoods, each within BARS["loglik"] of its own size
    slack = 2.0 * dc.BARS["loglik"] * 2.0 * (np.abs(host["loglik"][fine]) + np.abs(host["lr_brownian"][fine]) + 1.0)
    assert (np.abs(got["lr_brownian"][fine] - host["lr_brownian"][fine]) <= slack).all()
    # a number for sigma2: every row that is not filled is used
    num = T.estimate_track_diffusion(dm, model, SEQ_LEN, directed={"sigma2": 0.01}, **kw)
    assert num["directed"]["variances"] == 0.01 and num["directed"]["blur"] == 0.0 and torch.equal(num["directed"]["use"], ~filled)
    want = M.estimate_directed_ml(num["directed"]["positions"], offsets, 0.01, frames=fr, use=~filled, dt=DT)
    assert _bits(num["velocity_ml"], want["velocity"]) and _bits(num["lr_directed"], want["lr_brownian"])
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, directed={"sigma2": "crlb"}, **{**kw, "localization": None})
    with pytest.raises(ValueError, match="directed"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, directed={"exposure": 0.1}, **kw)
    with pytest.raises(ValueError, match="blur"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, directed={"blur": 0.3}, **kw)
