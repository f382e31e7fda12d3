"""GPU: the kernels of csrc/confined_ml.hip through the raw C-ABI inside the guarded, poisoned buffers of tests/abi_guard.py
and through ops, on the 60 ranges of tests/confined_ml_common.batch: mivit_track_confined_ml against the numpy restatement
(helpers/msd._confined_ml_numpy), which tests/test_confined_ml.py holds against the dense likelihood, a Nelder-Mead polish
and tracks drawn from the model; mivit_track_confined_loglik against the restatement; null arguments; that a range's outputs
are bitwise the same alone, in the batch and in every launch; hostile offsets; the empty problems and the error codes; and
the path that reaches the kernel from a movie, tracking.estimate_track_diffusion(confined=...).  The bars are in
confined_ml_common.BARS, with their origin."""
import ctypes
from functools import lru_cache, partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import confined_ml_common as cc
from abi_call import Call, bits_equal, check_all, same_results
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as G
from moleculardiffusion_mivit_amd.helpers import models as MD
from moleculardiffusion_mivit_amd.helpers import msd as M
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

F64, I32, U8 = torch.float64, torch.int32, torch.uint8
OUTS = M._CF_OUTS
ESTIMATES, BARS_STD = ("D_conf", "radius", "lambda"), ("D_conf_std", "radius_std", "lambda_std", "corr", "centre_std")
LOGLIK_AT_BAR = 1e-10         # mivit_track_confined_loglik against the restatement at the same parameters, relative


def shape_of(k, n):
    return (n, 2) if k.startswith("centre") else n


@lru_cache(maxsize=None)
def the_batch():
    return cc.batch()


def args_of(b, var=True, frames=True, use=True):
    return (b["pos"], b["var"] if var else None, b["frames"].astype(np.int64) if frames else None, b["use"] if use else None,
            b["offsets"], cc.BATCH_DT)


@lru_cache(maxsize=None)
def restatement():
    """computed once on the CPU; the tests read it and leave it as it is"""
    want = dict(zip(OUTS, M._confined_ml_numpy(*args_of(the_batch()))))
    assert (want["status"] == 0).sum() >= cc.MIN_STATUS_0
    return want


def inputs(c, b, raw_offsets=None, var=True, frames=True, use=True):
    raw = b["offsets"] if raw_offsets is None else raw_offsets
    return (c.inp("pos", b["pos"], F64), c.inp("var", b["var"], F64) if var else None,
            c.inp("frames", b["frames"], I32) if frames else None, c.inp("use", b["use"].astype(np.uint8), U8) if use else None,
            len(b["pos"]), c.inp("offsets", raw, I32), len(raw) - 1, cc.BATCH_DT)


def ml_call(b, mis=0, **kw):
    c = Call("mivit_track_confined_ml", mis)
    n = len(b["offsets"]) - 1
    c.run(*inputs(c, b, **kw), *(c.out(k, shape_of(k, n), I32 if k in ("n_increments", "status") else F64) for k in OUTS))
    return c


def loglik_call(b, mis=0, centre=True, **kw):
    c = Call("mivit_track_confined_loglik", mis)
    n = len(b["offsets"]) - 1
    c.run(*inputs(c, b, **kw), c.inp("D", b["D"], F64), c.inp("s2", b["s2"], F64),
          c.inp("centre", b["centre"], F64) if centre else None, c.out("loglik", n, F64))
    return c


def compare(got, want, names):
    """the outputs of the kernel (dict of arrays) against the restatement's, by the bars of confined_ml_common.BARS"""
    assert np.array_equal(got["status"], want["status"]), [(names[k], int(got["status"][k]), int(want["status"][k]))
                                                             for k in np.nonzero(got["status"] != want["status"])[0]]
    assert np.array_equal(got["n_increments"], want["n_increments"])
    fine = want["status"] == 0
    for k in OUTS[:10]:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert np.array_equal(np.isinf(got[k]), np.isinf(want[k])) and np.array_equal(got[k][np.isinf(want[k])], want[k][np.isinf(want[k])]), k
    finite = np.isfinite(want["loglik"])
    rel = np.abs(got["loglik"][finite] - want["loglik"][finite]) / np.abs(want["loglik"][finite])
    print(f"loglik: worst relative difference {rel.max():.3g} (bar {cc.BARS['loglik']:g})")
    assert (rel <= cc.BARS["loglik"]).all(), [names[k] for k in np.nonzero(finite)[0][rel > cc.BARS["loglik"]]]
    for k in ESTIMATES + BARS_STD:
        g, w = got[k][fine], want[k][fine]
        err = np.abs(g - w) / (1.0 if k == "corr" else np.abs(w))
        print(f"{k}: worst difference on the status-0 ranges {err.max():.3g} (bar {cc.BARS[k]:g})")
        assert (err <= cc.BARS[k]).all(), (k, [names[i] for i in np.nonzero(fine)[0][err > cc.BARS[k]]])
    err = np.abs(got["centre"][fine] - want["centre"][fine]) / want["centre_std"][fine]
    print(f"centre: worst difference in units of its standard error {err.max():.3g} (bar {cc.BARS['lambda']:g})")
    assert (err <= cc.BARS["lambda"]).all()


def test_the_batch_holds_every_status():
    b, want = the_batch(), restatement()
    assert len(b["names"]) == 60
    assert set(want["status"].tolist()) >= {0, 1, 2, 3, 4}
    inc = dict(zip(b["names"], want["n_increments"].tolist()))
    assert inc["4 rows"] == 3 and inc["5 rows"] == 4 and inc["300 rows"] == 299
    st = dict(zip(b["names"], want["status"].tolist()))
    assert st["4 rows"] == 1 and st["5 rows"] != 1 and st["straight walk"] == 2 and st["white noise"] == 3 and st["identical rows"] == 4


@pytest.mark.parametrize("mis", [0, 1])
def test_fit_through_the_raw_abi_against_the_restatement(mis):
    c = ml_call(the_batch(), mis)
    want = restatement()
    check_all(c, {"status": want["status"], "n_increments": want["n_increments"]})      # every entry written, no poison left
    for k in OUTS[:10]:
        assert not c.outs[k].unchanged().numpy().any(), k
    compare({k: c.outs[k].numpy() for k in OUTS}, want, the_batch()["names"])


def test_fit_through_ops_against_the_restatement():
    b = the_batch()
    dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("pos", "var", "frames", "use", "offsets", "D", "s2", "centre")}
    got = ops.track_confined_ml(dev["pos"], dev["offsets"].int(), dev["var"], dev["frames"], dev["use"], dt=cc.BATCH_DT)
    assert [g.dtype for g in got] == [F64] * 10 + [I32, I32] and got[7].shape == got[8].shape == (60, 2)
    compare({k: g.cpu().numpy() for k, g in zip(OUTS, got)}, restatement(), b["names"])
    raw = ml_call(b)
    for k, g in zip(OUTS, got):
        assert g.is_cuda and bits_equal(g.cpu().numpy(), raw.outs[k].numpy()), k
    # the front ends on CUDA tensors are these calls
    fit = M.estimate_confinement_ml(dev["pos"], dev["offsets"], dev["var"], frames=dev["frames"], use=dev["use"], dt=cc.BATCH_DT)
    for k, g in zip(OUTS, got):
        assert fit[k].is_cuda and bits_equal(fit[k].double().cpu().numpy(), g.double().cpu().numpy()), k
    assert fit["status"].dtype == fit["n_increments"].dtype == torch.int64
    brownian = M.estimate_diffusion_ml(dev["pos"], dev["offsets"], dev["var"], frames=dev["frames"], use=dev["use"], dt=cc.BATCH_DT)["loglik"]
    assert bits_equal(fit["lr_brownian"].cpu().numpy(), (2.0 * (got[9] - brownian)).cpu().numpy())
    lr = fit["lr_brownian"][fit["status"] == 0].cpu().numpy()
    assert (lr >= -1e-6).all(), lr.min()
    ll = M.confined_loglik(dev["pos"], dev["offsets"], dev["D"], dev["s2"], dev["centre"], dev["var"], frames=dev["frames"], use=dev["use"],
                           dt=cc.BATCH_DT)["loglik"]
    assert ll.is_cuda and bits_equal(ll.cpu().numpy(), loglik_call(b).outs["loglik"].numpy())
    with pytest.raises(ValueError, match="dt"):
        ops.track_confined_ml(dev["pos"], dev["offsets"].int(), dt=0.0)
    with pytest.raises(ValueError, match="offsets"):
        ops.track_confined_ml(dev["pos"], dev["offsets"].int()[:-1], dev["var"])
    with pytest.raises(ValueError, match="var"):
        ops.track_confined_ml(dev["pos"], dev["offsets"].int(), dev["var"][:-1])
    with pytest.raises(ValueError, match="D and s2"):
        ops.track_confined_loglik(dev["pos"], dev["offsets"].int(), dev["D"][:-1], dev["s2"])
    with pytest.raises(ValueError, match="centre"):
        ops.track_confined_loglik(dev["pos"], dev["offsets"].int(), dev["D"], dev["s2"], dev["centre"][:-1])


@pytest.mark.parametrize("centre", [True, False])
def test_loglik_against_the_restatement(centre):
    b = the_batch()
    c = loglik_call(b, mis=0 if centre else 1, centre=centre)
    got = c.outs["loglik"].numpy()
    assert not c.outs["loglik"].unchanged().numpy().any()
    want = M._confined_loglik_numpy(*args_of(b), b["D"], b["s2"], b["centre"] if centre else None)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 3 and np.isfinite(want).sum() >= 50   # 0 rows, 1 row, every row unusable
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    ok = np.isfinite(want)
    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
    print(f"centre given {centre}: worst relative difference of loglik to the restatement {rel.max():.3g} (bar {LOGLIK_AT_BAR:g})")
    assert (rel <= LOGLIK_AT_BAR).all()
    # parameters that are not positive and finite: NaN
    bad = dict(b, D=np.where(np.arange(60) % 2 == 0, -1.0, b["D"]), s2=np.where(np.arange(60) % 3 == 0, np.inf, b["s2"]))
    out = loglik_call(bad, centre=centre).outs["loglik"].numpy()
    off = (np.arange(60) % 2 == 0) | (np.arange(60) % 3 == 0)
    assert np.isnan(out[off]).all() and bits_equal(out[~off], got[~off])


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


def test_a_range_alone_is_the_range_in_the_batch():
    """n = 1 with the offsets of each range in turn, on the same device buffers: bitwise the batch's entry; and the batch twice"""
    b = the_batch()
    n = len(b["names"])
    first, second = ml_call(b), ml_call(b)
    same_results(first, second)
    ll_first, ll_second = loglik_call(b), loglik_call(b)
    same_results(ll_first, ll_second)
    dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("pos", "var", "frames", "D", "s2", "centre")}
    dev["use"] = torch.from_numpy(b["use"].astype(np.uint8)).cuda()
    off = torch.from_numpy(b["offsets"].astype(np.int32)).cuda()
    outs = {k: torch.zeros(shape_of(k, n), dtype=I32 if k in ("n_increments", "status") else F64, device="cuda") for k in OUTS}
    ll = torch.zeros(n, dtype=F64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = (p(dev["pos"]), p(dev["var"]), p(dev["frames"]), p(dev["use"]), len(b["pos"]))
    for k in range(n):
        N.check(N.lib.mivit_track_confined_ml(*rows, p(off[k:k + 2]), 1, cc.BATCH_DT, *(p(outs[o][k:k + 1]) for o in OUTS), stream),
                "mivit_track_confined_ml")
        N.check(N.lib.mivit_track_confined_loglik(*rows, p(off[k:k + 2]), 1, cc.BATCH_DT, p(dev["D"][k:k + 1]), p(dev["s2"][k:k + 1]),
                                                  p(dev["centre"][k:k + 1]), p(ll[k:k + 1]), stream), "mivit_track_confined_loglik")
    torch.cuda.synchronize()
    for o in OUTS:
        assert bits_equal(outs[o].cpu().numpy(), first.outs[o].numpy()), o
    assert bits_equal(ll.cpu().numpy(), ll_first.outs["loglik"].numpy())


def test_hostile_offsets_are_clamped():
    """the first offset below 0 and the last above N: the ranges keep their rows, nothing outside [0, N) is read"""
    import abi_guard as guard
    b = the_batch()
    raw = np.array(b["offsets"], np.int64)
    raw[0], raw[-1] = -3, len(b["pos"]) + 2
    hostile = guard.bounded(raw, 0, len(b["pos"]), 16)
    same_results(ml_call(b, raw_offsets=hostile), ml_call(b))
    same_results(loglik_call(b, raw_offsets=hostile), loglik_call(b))


def test_empty_problems_and_error_codes():
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = [None] * 4
    assert N.lib.mivit_track_confined_ml(*none, 0, None, 0, 1.0, *[None] * 12, stream) == 0
    assert N.lib.mivit_track_confined_loglik(*none, 0, None, 0, 1.0, None, None, None, None, stream) == 0
    c = Call("mivit_track_confined_ml")                                    # no rows, two ranges: both are empty
    c.run(*none, 0, c.inp("offsets", np.zeros(3, np.int64), I32), 2, 1.0,
          *(c.out(k, shape_of(k, 2), I32 if k in ("n_increments", "status") else F64) for k in OUTS))
    check_all(c, dict({k: np.full(shape_of(k, 2), np.nan) for k in OUTS[:10]}, n_increments=np.zeros(2), status=np.ones(2)))
    c = Call("mivit_track_confined_loglik")
    c.run(*none, 0, c.inp("offsets", np.zeros(3, np.int64), I32), 2, 1.0, c.inp("D", np.ones(2), F64), c.inp("s2", np.ones(2), F64), None,
          c.out("loglik", 2, F64))
    check_all(c, {"loglik": np.full(2, np.nan)})
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        assert N.lib.mivit_track_confined_ml(*none, 0, None, 0, dt, *[None] * 12, stream) != 0
        assert N.lib.mivit_track_confined_loglik(*none, 0, None, 0, dt, None, None, None, None, stream) != 0
    assert N.lib.mivit_track_confined_ml(*none, -1, None, 0, 1.0, *[None] * 12, stream) != 0
    off = torch.zeros(2, dtype=I32, device="cuda")
    assert N.lib.mivit_track_confined_ml(*none, 0, ctypes.c_void_p(off.data_ptr()), 1, 1.0, *[None] * 12, stream) != 0, "null outputs"
    assert N.lib.mivit_track_confined_ml(*none, 5, ctypes.c_void_p(off.data_ptr()), 1, 1.0, *[ctypes.c_void_p(off.data_ptr())] * 12, stream) != 0, "null pos"
    got = ops.track_confined_ml(torch.zeros(0, 2, dtype=F64, device="cuda"), torch.zeros(1, dtype=I32, device="cuda"))
    assert all(len(g) == 0 for g in got)
    assert len(ops.track_confined_loglik(torch.zeros(0, 2, dtype=F64, device="cuda"), torch.zeros(1, dtype=I32, device="cuda"),
                                         torch.zeros(0, dtype=F64, device="cuda"), torch.zeros(0, dtype=F64, device="cuda"))) == 0


# ----------------------------------------------------------------------------------------------------------------------
# estimate_track_diffusion(confined=)
# ----------------------------------------------------------------------------------------------------------------------
SEQ_LEN, PATCH, BATCH, DT = 5, 9, 16, 0.03
CAMERA = {"background": 10.0, "gain": 2.0, "offset": 100.0, "read_noise": 2.0}


def _bits(a, b):
    return a.dtype == b.dtype and bits_equal(a.double().cpu().numpy(), b.double().cpu().numpy())


def test_estimate_track_diffusion_with_confined():
    """the 4-particle, 30-frame, 96 x 96 camera movie of tests/test_likelihood_gpu.py, its particles in wells of radius 3"""
    movie, truth = G.simulate_movie(4, 30, 96, 96, 0.3, 4, image_props={"particle_intensity": [300.0, 5.0]}, camera=CAMERA,
                                    generator=torch.Generator().manual_seed(6), blink=0.1, confinement={"radius": 3.0})
    dm = movie.cuda()
    props = dict(G.DEFAULT_IMAGE_PROPS)
    loc = {"gain": CAMERA["gain"], "offset": CAMERA["offset"], "read_var": (CAMERA["read_noise"] / CAMERA["gain"]) ** 2,
           "sigma0": G.psf_sigma_hr(props) / props["upsampling_factor"]}
    torch.manual_seed(0)
    model = MD.GeneralTransformer(MD.LinearProjectionEmbedding, dict(patch_size=PATCH, embed_dim=64), 64, 4, 128, 1,
                                  partial(MD.MLPHead, hidden_dim=128, output_dim=1), F.relu, precision="fp32").cuda()
    kw = dict(patch_size=PATCH, dt=DT, batch_size=BATCH, min_track_length=5, max_gap=2, localization=loc)
    base = T.estimate_track_diffusion(dm, model, SEQ_LEN, **kw)
    none = T.estimate_track_diffusion(dm, model, SEQ_LEN, confined=None, **kw)
    res = T.estimate_track_diffusion(dm, model, SEQ_LEN, confined={}, **kw)
    new = {"radius_ml", "radius_ml_std", "D_conf", "lambda_ml", "lr_confined", "confined_status", "confined"}

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

    same(none, base)                                                       # confined=None: exactly today's keys and bits
    same(res, base, new)                                                   # ... and confined adds to them, changing none
    n_tracks = len(res["track_id"])
    assert n_tracks >= 3 and all(res[k].shape == (n_tracks,) for k in new - {"confined"})
    assert res["confined_status"].dtype == torch.int64
    table, _ = T.track_particles_tensors(dm, return_dog=False, min_track_length=5, max_gap=2)
    fr, y, x, tid, offsets, filled = T.tracks_table_by_track(table)
    fit = T.refine_localizations_tensors(T.extract_patches_flat(dm.float(), fr, y, x, PATCH), y, x, method="mle", camera=loc)
    cf = res["confined"]
    assert set(cf) == {"positions", "variances", "frames", "use"}
    assert _bits(cf["positions"], torch.stack([fit["y_refined"], fit["x_refined"]], dim=1))
    assert _bits(cf["variances"], torch.stack([fit["y_std"] ** 2, fit["x_std"] ** 2], dim=1))
    assert torch.equal(cf["frames"], fr) and torch.equal(cf["use"], (fit["status"] == 0) & ~filled)
    want = M.estimate_confinement_ml(cf["positions"], offsets, cf["variances"], frames=cf["frames"], use=cf["use"], dt=DT)
    for k, key in (("radius_ml", "radius"), ("radius_ml_std", "radius_std"), ("D_conf", "D_conf"), ("lambda_ml", "lambda"),
                   ("lr_confined", "lr_brownian"), ("confined_status", "status")):
        assert _bits(res[k], want[key]), k
    print("status", res["confined_status"].tolist(), "radius_ml", res["radius_ml"].cpu().numpy().round(3).tolist(),
          "lr_confined", res["lr_confined"].cpu().numpy().round(2).tolist())
    # a number for sigma2: every row that is not filled is used
    num = T.estimate_track_diffusion(dm, model, SEQ_LEN, confined={"sigma2": 0.01}, **kw)
    assert num["confined"]["variances"] == 0.01 and torch.equal(num["confined"]["use"], ~filled)
    want = M.estimate_confinement_ml(num["confined"]["positions"], offsets, 0.01, frames=fr, use=~filled, dt=DT)
    assert _bits(num["radius_ml"], want["radius"]) and _bits(num["lr_confined"], want["lr_brownian"])
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, confined={"sigma2": "crlb"}, **{**kw, "localization": None})
    with pytest.raises(ValueError, match="confined"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, confined={"blur": 0.1}, **kw)
