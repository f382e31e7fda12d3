"""GPU: the kernel of csrc/likelihood.hip (ops.track_diffusion_ml, mivit_track_diffusion_ml) against the numpy restatement
(helpers/msd._diffusion_ml_numpy), which tests/test_likelihood.py holds against a dense likelihood and against tracks drawn
from the model, on the 67 ranges of tests/likelihood_common.batch: through ops, and through the raw C-ABI inside the guarded,
poisoned buffers of tests/abi_guard.py; that a range's outputs are bitwise the same alone, in the batch and in every launch;
and the paths that reach the kernel, helpers/msd.estimate_diffusion_ml on CUDA tensors and
tracking.estimate_track_diffusion(ml=...).  The bars are in likelihood_common.BARS, with their origin."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import likelihood_common as lc
from abi_call import Call, bits_equal, check_all, same_results
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as G
from moleculardiffusion_mivit_amd.helpers import models as MD
from moleculardiffusion_mivit_amd.helpers import msd as M
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

F64, I32, U8 = torch.float64, torch.int32, torch.uint8
OUTS = ("D", "D_std", "loglik", "n_increments", "status")
CLOSE = {k: lc.close(v) for k, v in lc.BARS.items()}


@pytest.fixture(scope="module")
def batch():
    return lc.batch()


def restatement(b, var=True, frames=True, use=True):
    got = M._diffusion_ml_numpy(b["pos"], b["var"] if var else None, b["frames"].astype(np.int64) if frames else None,
                                b["use"] if use else None, b["offsets"], lc.BATCH_DT, lc.BATCH_R)
    return dict(zip(OUTS, got))


@pytest.fixture(scope="module")
def reference(batch):
    """computed once; the tests below read it and leave it as it is"""
    return restatement(batch)


def ml_call(b, raw_offsets=None, var=True, frames=True, use=True, mis=0):
    c = Call("mivit_track_diffusion_ml", mis)
    raw = b["offsets"] if raw_offsets is None else raw_offsets
    n = len(raw) - 1
    c.run(c.inp("pos", b["pos"], F64), c.inp("var", b["var"], F64) if var else None,
          c.inp("frames", b["frames"], I32) if frames else None, c.inp("use", b["use"].astype(np.uint8), U8) if use else None,
          len(b["pos"]), c.inp("offsets", raw, I32), n, lc.BATCH_DT, lc.BATCH_R, c.out("D", n, F64), c.out("D_std", n, F64),
          c.out("loglik", n, F64), c.out("n_increments", n, I32), c.out("status", n, I32))
    return c


def test_the_batch_holds_every_status(reference):
    assert sorted(set(reference["status"].tolist())) == [0, 1, 2]
    assert (reference["status"] == 0).sum() > 40


@pytest.mark.parametrize("mis", [0, 1])
def test_c_abi_in_guarded_buffers_against_the_restatement(batch, reference, mis):
    c = ml_call(batch, mis=mis)
    for k in ("D", "D_std", "loglik"):
        got, want = c.outs[k].numpy(), reference[k]
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where((got == want) | np.isnan(want), 0.0, np.abs(got - want) / np.abs(want))
        print(f"{k}: worst relative difference {np.nanmax(rel):.3g} (bar {lc.BARS[k]:g})")
    check_all(c, reference, close=CLOSE)                                   # status and n_increments bitwise


@pytest.mark.parametrize("var,frames,use", [(False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_null_arguments_are_the_defaults(batch, var, frames, use):
    b = dict(batch)
    if not use:                                                            # without flags every row counts: keep them finite
        b["pos"] = np.where(np.isfinite(b["pos"]), b["pos"], 1.0)
        b["var"] = np.where(np.isfinite(b["var"]) & (b["var"] >= 0), b["var"], 0.01)
    c = ml_call(b, var=var, frames=frames, use=use)
    check_all(c, restatement(b, var, frames, use), close=CLOSE)
    n = len(b["pos"])
    full = dict(b, var=b["var"] if var else np.zeros((n, 2)), use=b["use"] if use else np.ones(n, bool),
                frames=b["frames"] if frames else np.concatenate([np.arange(e - a) for a, e in zip(b["offsets"][:-1], b["offsets"][1:])]))
    same_results(c, ml_call(full))


def test_ops_against_the_restatement(batch, reference):
    dev = {k: torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in ("pos", "var", "frames", "use", "offsets")}
    args = (dev["pos"], dev["offsets"].int(), dev["var"], dev["frames"], dev["use"])
    got = ops.track_diffusion_ml(*args, dt=lc.BATCH_DT, blur=lc.BATCH_R)
    again = ops.track_diffusion_ml(*args, dt=lc.BATCH_DT, blur=lc.BATCH_R)
    assert [g.dtype for g in got] == [F64, F64, F64, I32, I32]
    for k, g, a in zip(OUTS, got, again):
        assert g.is_cuda and bits_equal(g.cpu().numpy(), a.cpu().numpy()), k
        if k in CLOSE:
            CLOSE[k](g.cpu().numpy(), reference[k], k)
        else:
            assert np.array_equal(g.cpu().numpy(), reference[k]), k
    # the front end on CUDA tensors is this call
    fit = M.estimate_diffusion_ml(dev["pos"], dev["offsets"], dev["var"], frames=dev["frames"], use=dev["use"], dt=lc.BATCH_DT,
                                  blur=lc.BATCH_R)
    for key, k in (("D_ml", 0), ("D_ml_std", 1), ("loglik", 2), ("n_increments", 3), ("status", 4)):
        assert fit[key].is_cuda and bits_equal(fit[key].double().cpu().numpy(), got[k].double().cpu().numpy()), key
    assert fit["status"].dtype == fit["n_increments"].dtype == torch.int64
    with pytest.raises(ValueError, match="blur"):
        ops.track_diffusion_ml(*args, blur=0.3)
    with pytest.raises(ValueError, match="offsets"):
        ops.track_diffusion_ml(dev["pos"], dev["offsets"].int()[:-1], dev["var"])
    with pytest.raises(ValueError, match="var"):
        ops.track_diffusion_ml(dev["pos"], dev["offsets"].int(), dev["var"][:-1])


def test_a_range_alone_is_the_range_in_the_batch(batch):
    """n = 1 with the offsets of each range in turn, on the same device buffers: bitwise the batch's entry; and the batch twice"""
    first, second = ml_call(batch), ml_call(batch)
    same_results(first, second)
    whole = {k: first.outs[k].numpy() for k in OUTS}
    dev = {k: torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in ("pos", "var", "frames")}
    dev["use"] = torch.from_numpy(batch["use"].astype(np.uint8)).cuda()
    off = torch.from_numpy(batch["offsets"].astype(np.int32)).cuda()
    outs = {k: torch.zeros(lc.BATCH_N, dtype=I32 if k in ("n_increments", "status") else F64, device="cuda") for k in OUTS}
    p = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in range(lc.BATCH_N):
        N.check(N.lib.mivit_track_diffusion_ml(p(dev["pos"]), p(dev["var"]), p(dev["frames"]), p(dev["use"]), len(batch["pos"]),
                                               p(off[k:k + 2]), 1, lc.BATCH_DT, lc.BATCH_R, *(p(outs[o][k:k + 1]) for o in OUTS),
                                               stream), "mivit_track_diffusion_ml")
    torch.cuda.synchronize()
    for o in OUTS:
        assert bits_equal(outs[o].cpu().numpy(), whole[o]), o


def test_hostile_offsets_are_clamped(batch, reference):
    """the first offset below 0 and the last above N: the ranges keep their rows, nothing outside [0, N) is read"""
    import abi_guard as guard
    raw = np.array(batch["offsets"], np.int64)
    raw[0], raw[-1] = -3, len(batch["pos"]) + 2
    c = ml_call(batch, raw_offsets=guard.bounded(raw, 0, len(batch["pos"]), 16))
    check_all(c, reference, close=CLOSE)
    same_results(c, ml_call(batch))


def test_empty_problems():
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert N.lib.mivit_track_diffusion_ml(None, None, None, None, 0, None, 0, 1.0, 0.0, None, None, None, None, None, stream) == 0
    c = Call("mivit_track_diffusion_ml")                                   # no rows, two ranges: both are empty
    c.run(None, None, None, None, 0, c.inp("offsets", np.zeros(3, np.int64), I32), 2, 1.0, 0.0, c.out("D", 2, F64),
          c.out("D_std", 2, F64), c.out("loglik", 2, F64), c.out("n_increments", 2, I32), c.out("status", 2, I32))
    nan = np.full(2, np.nan)
    check_all(c, {"D": nan, "D_std": nan, "loglik": nan, "n_increments": np.zeros(2), "status": np.ones(2)})
    for bad in ((1.0, 0.3), (0.0, 0.1)):
        assert N.lib.mivit_track_diffusion_ml(None, None, None, None, 0, None, 0, *bad, None, None, None, None, None, stream) != 0
    got = ops.track_diffusion_ml(torch.zeros(0, 2, dtype=F64, device="cuda"), torch.zeros(1, dtype=I32, device="cuda"))
    assert all(len(g) == 0 for g in got)


# ----------------------------------------------------------------------------------------------------------------------
# estimate_track_diffusion(ml=)
# ----------------------------------------------------------------------------------------------------------------------
SEQ_LEN, PATCH, BATCH, DT = 5, 9, 16, 0.03
CAMERA = {"background": 10.0, "gain": 2.0, "offset": 100.0, "read_noise": 2.0}


def _bits(a, b):
    return a.dtype == b.dtype and bits_equal(a.double().cpu().numpy(), b.double().cpu().numpy())


def test_estimate_track_diffusion_with_ml():
    """the movie of tests/test_localize_gpu.py::test_estimate_track_diffusion_with_localization, with blinking particles so
    that gap closing has rows to fill"""
    movie, truth = G.simulate_movie(4, 30, 96, 96, 0.3, 4, image_props={"particle_intensity": [300.0, 5.0]}, camera=CAMERA,
                                    generator=torch.Generator().manual_seed(6), blink=0.1)
    dm = movie.cuda()
    props = dict(G.DEFAULT_IMAGE_PROPS)
    loc = {"gain": CAMERA["gain"], "offset": CAMERA["offset"], "read_var": (CAMERA["read_noise"] / CAMERA["gain"]) ** 2,
           "sigma0": G.psf_sigma_hr(props) / props["upsampling_factor"]}
    torch.manual_seed(0)
    model = MD.GeneralTransformer(MD.LinearProjectionEmbedding, dict(patch_size=PATCH, embed_dim=64), 64, 4, 128, 1,
                                  partial(MD.MLPHead, hidden_dim=128, output_dim=1), F.relu, precision="fp32").cuda()
    kw = dict(patch_size=PATCH, dt=DT, batch_size=BATCH, min_track_length=5, max_gap=2, localization=loc, segment={},
              states={"K": 2})
    base = T.estimate_track_diffusion(dm, model, SEQ_LEN, **kw)
    none = T.estimate_track_diffusion(dm, model, SEQ_LEN, ml=None, **kw)
    res = T.estimate_track_diffusion(dm, model, SEQ_LEN, ml={"blur": 1.0 / 6.0}, **kw)
    new = {"D_ml", "D_ml_std", "ml_status"}

    def same(a, b, extra=frozenset(), nested=frozenset()):
        """a holds what b holds, bit for bit, and the keys `extra` (`nested`: in its segments and states) besides"""
        assert set(a) == set(b) | extra
        for k, v in b.items():
            if isinstance(v, dict):
                same(a[k], v, nested if k in ("segments", "states") else frozenset())
            elif torch.is_tensor(v):
                assert _bits(a[k], v), k
            elif isinstance(v, np.ndarray):
                assert bits_equal(a[k], v), k
            else:
                assert a[k] == v or (a[k] != a[k] and v != v), k

    same(none, base)                                                       # ml=None: exactly today's keys and values
    same(res, base, new | {"ml"}, new)                                     # ... and ml adds to them, changing none
    n_tracks = len(res["track_id"])
    assert n_tracks >= 3 and res["D_ml"].shape == res["D_ml_std"].shape == res["ml_status"].shape == (n_tracks,)
    # the pieces by hand: the refined positions, the squared bounds, the frames, converged and not filled
    table, _ = T.track_particles_tensors(dm, return_dog=False, min_track_length=5, max_gap=2)
    fr, y, x, tid, offsets, filled = T.tracks_table_by_track(table)
    assert bool(filled.any()), "the case has filled rows"
    fit = T.refine_localizations_tensors(T.extract_patches_flat(dm.float(), fr, y, x, PATCH), y, x, method="mle", camera=loc)
    ml = res["ml"]
    assert set(ml) == {"positions", "variances", "frames", "use", "blur"} and ml["blur"] == 1.0 / 6.0
    assert _bits(ml["positions"], torch.stack([fit["y_refined"], fit["x_refined"]], dim=1))
    assert _bits(ml["variances"], torch.stack([fit["y_std"] ** 2, fit["x_std"] ** 2], dim=1))
    assert torch.equal(ml["frames"], fr) and torch.equal(ml["use"], (fit["status"] == 0) & ~filled)
    call = partial(M.estimate_diffusion_ml, ml["positions"], variances=ml["variances"], frames=ml["frames"], use=ml["use"], dt=DT,
                   blur=ml["blur"])
    for where, csr in ((res, offsets), (res["segments"], res["segments"]["seg_offsets"]), (res["states"], res["states"]["run_offsets"])):
        want = call(csr)
        assert len(want["D_ml"]) == len(csr) - 1
        for k, key in (("D_ml", "D_ml"), ("D_ml_std", "D_ml_std"), ("ml_status", "status")):
            assert _bits(where[k], want[key]), k
    st = res["ml_status"].cpu().numpy()
    print("status", st.tolist(), "D_ml", res["D_ml"].cpu().numpy().round(4).tolist(), "D_msd", res["D_msd"].cpu().numpy().round(4).tolist())
    assert (st == 0).sum() >= 3
    # a number for sigma2: every row that is not filled is used
    num = T.estimate_track_diffusion(dm, model, SEQ_LEN, ml={"sigma2": 0.01}, **kw)
    assert num["ml"]["variances"] == 0.01 and torch.equal(num["ml"]["use"], ~filled) and num["ml"]["blur"] == 0.0
    want = M.estimate_diffusion_ml(num["ml"]["positions"], offsets, 0.01, frames=fr, use=~filled, dt=DT)
    assert _bits(num["D_ml"], want["D_ml"]) and _bits(num["D_ml_std"], want["D_ml_std"])
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, ml={"sigma2": "crlb"}, **{**kw, "localization": None})
