"""GPU: the kernels of csrc/fbm_ml.hip through the raw C-ABI inside the guarded, poisoned buffers of tests/abi_guard.py, on the
40 ranges of tests/fbm_ml_common.batch: mivit_track_fbm_loglik against the dense fp64 statement of the likelihood (the
explicit matrix from the structure function at 50 digits, slogdet and solve), mivit_track_fbm_ml against the numpy
restatement (helpers/msd._fbm_ml_numpy), which tests/test_fbm_ml.py holds against Nelder-Mead and against tracks drawn from
the model; that a range's outputs are bitwise the same alone, in the batch and in every launch; the empty problems and the
error codes; and the path that reaches the kernel from a movie, tracking.estimate_track_diffusion(anomalous=...).  The bars
are in fbm_ml_common.BARS, with their origin."""
import ctypes
from functools import lru_cache, partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fbm_ml_common as fc
from abi_call import Call, bits_equal, check_all, same_results
from moleculardiffusion_mivit_amd import _native as N
from moleculardiffusion_mivit_amd import ops
from moleculardiffusion_mivit_amd.helpers import generation as G
from moleculardiffusion_mivit_amd.helpers import models as MD
from moleculardiffusion_mivit_amd.helpers import msd as M
from moleculardiffusion_mivit_amd.helpers import tracking as T

pytestmark = pytest.mark.gpu

F64, I32, U8 = torch.float64, torch.int32, torch.uint8
LL_OUTS = ("loglik", "n_increments", "status")
ML_OUTS = ("alpha", "alpha_std", "D", "D_std", "corr", "loglik", "n_increments", "status")
CLOSE = {"alpha": fc.close(fc.BARS["alpha"], relative=False), "D": fc.close(fc.BARS["D"]),
         "loglik": fc.close(fc.BARS["loglik"], relative=False), "alpha_std": fc.close(fc.BARS["alpha_std"]),
         "D_std": fc.close(fc.BARS["D_std"]), "corr": fc.close(1e-2, relative=False)}
EXPOSURES = (0.0, 0.25, 1.0)


@lru_cache(maxsize=None)
def the_batch():
    return fc.batch()


def args_of(b, var=True, frames=True, use=True):
    return (b["pos"], b["var"] if var else None, b["frames"].astype(np.int64) if frames else None, b["use"] if use else None,
            b["offsets"], fc.BATCH_DT)


@lru_cache(maxsize=None)
def restatement(E):
    """computed once per exposure; the tests read it and leave it as it is"""
    return dict(zip(ML_OUTS, M._fbm_ml_numpy(*args_of(the_batch()), E)))


def inputs(c, b, raw_offsets=None, var=True, frames=True, use=True):
    raw = b["offsets"] if raw_offsets is None else raw_offsets
    return (c.inp("pos", b["pos"], F64), c.inp("var", b["var"], F64) if var else None,
            c.inp("frames", b["frames"], I32) if frames else None, c.inp("use", b["use"].astype(np.uint8), U8) if use else None,
            len(b["pos"]), c.inp("offsets", raw, I32), len(raw) - 1, fc.BATCH_DT)


def loglik_call(b, E, mis=0, **kw):
    c = Call("mivit_track_fbm_loglik", mis)
    n = len(b["offsets"]) - 1
    c.run(*inputs(c, b, **kw), E, c.inp("alpha", b["alpha"], F64), c.inp("D", b["D"], F64), c.out("loglik", n, F64),
          c.out("n_increments", n, I32), c.out("status", n, I32))
    return c


def ml_call(b, E, mis=0, **kw):
    c = Call("mivit_track_fbm_ml", mis)
    n = len(b["offsets"]) - 1
    ws = c.work(n * ops.FBM_ML_WS_BYTES)
    c.run(*inputs(c, b, **kw), E, *(c.out(k, n, I32 if k in ("n_increments", "status") else F64) for k in ML_OUTS), ws, ws.nbytes)
    return c


def test_the_batch_holds_every_status_but_the_upper_end():
    want = restatement(1.0)
    assert set(want["status"].tolist()) >= {0, 1, 2, 5}
    assert (want["status"] == 0).sum() >= 20
    assert ops.FBM_ML_MAX_ROWS == fc.MAX_ROWS == M.FBM_ML_MAX_ROWS and ops.FBM_ML_MAX_SPAN == M.FBM_ML_MAX_SPAN


@pytest.mark.parametrize("E", EXPOSURES)
def test_loglik_against_the_dense_statement(E):
    b = the_batch()
    c = loglik_call(b, E, mis=1 if E == 0.25 else 0)
    got = c.outs["loglik"].numpy()
    _, n_inc, status = M._fbm_loglik_numpy(*args_of(b), E, b["alpha"], b["D"])
    check_all(c, {"n_increments": n_inc, "status": status})
    assert set(status.tolist()) == {0, 1, 5}
    worst = 0.0
    for k in range(len(status)):
        if status[k]:
            assert np.isnan(got[k]), b["names"][k]
            continue
        want = fc.dense_loglik(*fc.usable_rows(b, k), b["alpha"][k], b["D"][k], fc.BATCH_DT, E)
        if not np.isfinite(want):                                         # motionless without variance: the matrix is singular
            assert got[k] == want, b["names"][k]
            continue
        rel = abs(got[k] - want) / abs(want)
        worst = max(worst, rel)
        assert rel <= fc.LOGLIK_BAR, (b["names"][k], got[k], want)
    print(f"exposure {E}: worst relative difference of loglik to the dense statement {worst:.3g} (bar {fc.LOGLIK_BAR:g})")


@pytest.mark.parametrize("E", EXPOSURES)
def test_fit_against_the_restatement(E):
    c = ml_call(the_batch(), E, mis=1 if E == 0.25 else 0)
    want = restatement(E)
    for k in ("alpha", "D", "loglik", "alpha_std", "D_std", "corr"):
        got = c.outs[k].numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got - want[k]) / (np.abs(want[k]) if k in ("D", "alpha_std", "D_std") else 1.0)
        err = np.where((got == want[k]) | np.isnan(want[k]), 0.0, err)
        print(f"exposure {E}: {k}: worst difference {np.nanmax(err):.3g} at {the_batch()['names'][int(np.nanargmax(err))]}")
    check_all(c, want, close=CLOSE)                                       # status and n_increments bitwise


@pytest.mark.parametrize("var,frames,use", [(False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_null_arguments_are_the_defaults(var, frames, use):
    b = dict(the_batch())
    if not use:                                                            # without flags every row counts: keep them finite
        b["pos"] = np.where(np.isfinite(b["pos"]), b["pos"], 1.0)
        b["var"] = np.where(np.isfinite(b["var"]) & (b["var"] >= 0), b["var"], 0.01)
    n = len(b["pos"])
    full = dict(b, var=b["var"] if var else np.zeros((n, 2)), use=b["use"] if use else np.ones(n, bool),
                frames=b["frames"] if frames else np.concatenate([np.arange(e - a) for a, e in zip(b["offsets"][:-1], b["offsets"][1:])]))
    same_results(ml_call(b, 1.0, var=var, frames=frames, use=use), ml_call(full, 1.0))
    same_results(loglik_call(b, 1.0, var=var, frames=frames, use=use), loglik_call(full, 1.0))


def test_a_range_alone_is_the_range_in_the_batch():
    """n = 1 with the offsets of each range in turn, on the same device buffers: bitwise the batch's entry; and the batch twice"""
    b = the_batch()
    n, E = len(b["names"]), 1.0
    first, second = ml_call(b, E), ml_call(b, E)
    same_results(first, second)
    ll_first, ll_second = loglik_call(b, E), loglik_call(b, E)
    same_results(ll_first, ll_second)
    dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("pos", "var", "frames", "alpha", "D")}
    dev["use"] = torch.from_numpy(b["use"].astype(np.uint8)).cuda()
    off = torch.from_numpy(b["offsets"].astype(np.int32)).cuda()
    outs = {k: torch.zeros(n, dtype=I32 if k in ("n_increments", "status") else F64, device="cuda") for k in ML_OUTS}
    ll_outs = {k: torch.zeros(n, dtype=I32 if k in ("n_increments", "status") else F64, device="cuda") for k in LL_OUTS}
    ws = torch.zeros(ops.FBM_ML_WS_BYTES // 8, dtype=F64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = (p(dev["pos"]), p(dev["var"]), p(dev["frames"]), p(dev["use"]), len(b["pos"]))
    for k in range(n):
        N.check(N.lib.mivit_track_fbm_ml(*rows, p(off[k:k + 2]), 1, fc.BATCH_DT, E, *(p(outs[o][k:k + 1]) for o in ML_OUTS), p(ws),
                                         ws.numel() * 8, stream), "mivit_track_fbm_ml")
        N.check(N.lib.mivit_track_fbm_loglik(*rows, p(off[k:k + 2]), 1, fc.BATCH_DT, E, p(dev["alpha"][k:k + 1]), p(dev["D"][k:k + 1]),
                                             *(p(ll_outs[o][k:k + 1]) for o in LL_OUTS), stream), "mivit_track_fbm_loglik")
    torch.cuda.synchronize()
    for o in ML_OUTS:
        assert bits_equal(outs[o].cpu().numpy(), first.outs[o].numpy()), o
    for o in LL_OUTS:
        assert bits_equal(ll_outs[o].cpu().numpy(), ll_first.outs[o].numpy()), o


def test_ops_and_the_front_ends():
    b, E = the_batch(), 1.0
    dev = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("pos", "var", "frames", "use", "offsets", "alpha", "D")}
    got = ops.track_fbm_ml(dev["pos"], dev["offsets"].int(), dev["var"], dev["frames"], dev["use"], dt=fc.BATCH_DT, exposure=E)
    assert [g.dtype for g in got] == [F64] * 6 + [I32, I32]
    raw = ml_call(b, E)
    for k, g in zip(ML_OUTS, got):
        assert g.is_cuda and bits_equal(g.cpu().numpy(), raw.outs[k].numpy()), k
    fit = M.estimate_anomalous_ml(dev["pos"], dev["offsets"], dev["var"], frames=dev["frames"], use=dev["use"], dt=fc.BATCH_DT, exposure=E)
    for key, k in (("alpha_ml", 0), ("alpha_ml_std", 1), ("D_alpha", 2), ("D_alpha_std", 3), ("corr", 4), ("loglik", 5),
                   ("n_increments", 6), ("status", 7)):
        assert fit[key].is_cuda and bits_equal(fit[key].double().cpu().numpy(), got[k].double().cpu().numpy()), key
    assert fit["status"].dtype == fit["n_increments"].dtype == torch.int64
    brownian = M.estimate_diffusion_ml(dev["pos"], dev["offsets"], dev["var"], frames=dev["frames"], use=dev["use"], dt=fc.BATCH_DT,
                                       blur=E / 6.0)["loglik"]
    assert bits_equal(fit["lr_brownian"].cpu().numpy(), (2.0 * (got[5] - brownian)).cpu().numpy())
    lr = fit["lr_brownian"][fit["status"] == 0].cpu().numpy()
    assert (lr >= -1e-6).all(), lr.min()
    ll = M.fbm_loglik(dev["pos"], dev["offsets"], dev["alpha"], dev["D"], dev["var"], frames=dev["frames"], use=dev["use"],
                      dt=fc.BATCH_DT, exposure=E)
    raw = loglik_call(b, E)
    for k in LL_OUTS:
        assert ll[k].is_cuda and bits_equal(ll[k].double().cpu().numpy(), raw.outs[k].numpy().astype(np.float64)), k
    with pytest.raises(ValueError, match="exposure"):
        ops.track_fbm_ml(dev["pos"], dev["offsets"].int(), exposure=1.5)
    with pytest.raises(ValueError, match="offsets"):
        ops.track_fbm_ml(dev["pos"], dev["offsets"].int()[:-1], dev["var"])
    with pytest.raises(ValueError, match="alpha"):
        ops.track_fbm_loglik(dev["pos"], dev["offsets"].int(), dev["alpha"][:-1], dev["D"])


def test_empty_problems_and_error_codes():
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = [None] * 4
    assert N.lib.mivit_track_fbm_loglik(*none, 0, None, 0, 1.0, 0.0, None, None, None, None, None, stream) == 0
    assert N.lib.mivit_track_fbm_ml(*none, 0, None, 0, 1.0, 0.0, *[None] * 8, None, 0, stream) == 0
    c = Call("mivit_track_fbm_ml")                                         # no rows, two ranges: both are empty
    ws = c.work(2 * ops.FBM_ML_WS_BYTES)
    c.run(*none, 0, c.inp("offsets", np.zeros(3, np.int64), I32), 2, 1.0, 0.5,
          *(c.out(k, 2, I32 if k in ("n_increments", "status") else F64) for k in ML_OUTS), ws, ws.nbytes)
    nan = np.full(2, np.nan)
    check_all(c, dict({k: nan for k in ML_OUTS[:6]}, n_increments=np.zeros(2), status=np.ones(2)))
    c = Call("mivit_track_fbm_loglik")
    c.run(*none, 0, c.inp("offsets", np.zeros(3, np.int64), I32), 2, 1.0, 0.5, c.inp("alpha", np.ones(2), F64),
          c.inp("D", np.ones(2), F64), c.out("loglik", 2, F64), c.out("n_increments", 2, I32), c.out("status", 2, I32))
    check_all(c, {"loglik": nan, "n_increments": np.zeros(2), "status": np.ones(2)})
    for dt, E in ((0.0, 0.5), (float("inf"), 0.5), (1.0, -0.1), (1.0, 1.5), (1.0, float("nan"))):
        assert N.lib.mivit_track_fbm_loglik(*none, 0, None, 0, dt, E, None, None, None, None, None, stream) != 0
        assert N.lib.mivit_track_fbm_ml(*none, 0, None, 0, dt, E, *[None] * 8, None, 0, stream) != 0
    off = torch.zeros(2, dtype=I32, device="cuda")
    out = torch.zeros(8, dtype=F64, device="cuda")
    p = ctypes.c_void_p(out.data_ptr())
    small = N.lib.mivit_track_fbm_ml(*none, 0, ctypes.c_void_p(off.data_ptr()), 1, 1.0, 0.0, *[p] * 8, p, ops.FBM_ML_WS_BYTES - 8, stream)
    assert small != 0, "a workspace that is too small is an error"
    got = ops.track_fbm_ml(torch.zeros(0, 2, dtype=F64, device="cuda"), torch.zeros(1, dtype=I32, device="cuda"))
    assert all(len(g) == 0 for g in got)
    # parameters outside their range: status 6, nothing else happens
    b = the_batch()
    k = b["names"].index("33 rows")
    pos = torch.from_numpy(np.ascontiguousarray(b["pos"][b["offsets"][k]:b["offsets"][k + 1]])).cuda()
    offs = torch.tensor([0, len(pos)], dtype=I32, device="cuda")
    for a, D in ((0.0, 0.1), (2.0, 0.1), (float("nan"), 0.1), (1.0, -0.1), (1.0, float("inf"))):
        ll, _, st = ops.track_fbm_loglik(pos, offs, torch.tensor([a], dtype=F64, device="cuda"), torch.tensor([D], dtype=F64, device="cuda"))
        assert int(st[0]) == 6 and bool(torch.isnan(ll[0]))


# ----------------------------------------------------------------------------------------------------------------------
# estimate_track_diffusion(anomalous=)
# ----------------------------------------------------------------------------------------------------------------------
SEQ_LEN, PATCH, BATCH, DT = 5, 9, 16, 0.03


def _bits(a, b):
    return a.dtype == b.dtype and bits_equal(a.double().cpu().numpy(), b.double().cpu().numpy())


def test_estimate_track_diffusion_with_anomalous():
    movie, truth = G.simulate_movie(4, 40, 64, 64, 0.3, 4, alphas=torch.tensor([0.6, 1.0, 1.4, 1.0], dtype=torch.float64), generator=torch.Generator().manual_seed(3),
                                    blink=0.1)
    dm = movie.cuda()
    torch.manual_seed(0)
    model = MD.GeneralTransformer(MD.LinearProjectionEmbedding, dict(patch_size=PATCH, embed_dim=64), 64, 4, 128, 1,
                                  partial(MD.MLPHead, hidden_dim=128, output_dim=1), F.relu, precision="fp32").cuda()
    kw = dict(patch_size=PATCH, dt=DT, batch_size=BATCH, min_track_length=5, max_gap=2)
    base = T.estimate_track_diffusion(dm, model, SEQ_LEN, **kw)
    none = T.estimate_track_diffusion(dm, model, SEQ_LEN, anomalous=None, **kw)
    res = T.estimate_track_diffusion(dm, model, SEQ_LEN, anomalous={"exposure": 1.0, "sigma2": 0.01}, **kw)
    new = {"alpha_ml", "alpha_ml_std", "D_alpha", "anomalous_status", "anomalous"}
    assert set(none) == set(base) and set(res) == set(base) | new
    for k, v in base.items():
        for other in (none, res):
            if torch.is_tensor(v):
                assert _bits(other[k], v), k
            elif isinstance(v, np.ndarray):
                assert bits_equal(other[k], v), k
            else:
                assert other[k] == v, k
    n_tracks = len(res["track_id"])
    assert n_tracks >= 3 and res["alpha_ml"].shape == res["alpha_ml_std"].shape == res["D_alpha"].shape == (n_tracks,)
    assert res["anomalous_status"].dtype == torch.int64
    table, _ = T.track_particles_tensors(dm, return_dog=False, min_track_length=5, max_gap=2)
    fr, y, x, tid, offsets, filled = T.tracks_table_by_track(table)
    an = res["anomalous"]
    assert set(an) == {"positions", "variances", "frames", "use", "exposure"} and an["exposure"] == 1.0 and an["variances"] == 0.01
    assert torch.equal(an["frames"], fr) and torch.equal(an["use"], ~filled)
    want = M.estimate_anomalous_ml(an["positions"], offsets, an["variances"], frames=an["frames"], use=an["use"], dt=DT,
                                   exposure=an["exposure"])
    for k, key in (("alpha_ml", "alpha_ml"), ("alpha_ml_std", "alpha_ml_std"), ("D_alpha", "D_alpha"), ("anomalous_status", "status")):
        assert _bits(res[k], want[key]), k
    print("status", res["anomalous_status"].tolist(), "alpha_ml", res["alpha_ml"].cpu().numpy().round(3).tolist())
    assert int((res["anomalous_status"] == 0).sum()) >= 2
    with pytest.raises(ValueError, match="crlb"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, anomalous={"sigma2": "crlb"}, **kw)
    with pytest.raises(ValueError, match="exposure"):
        T.estimate_track_diffusion(dm, model, SEQ_LEN, anomalous={"exposure": 2.0}, **kw)
