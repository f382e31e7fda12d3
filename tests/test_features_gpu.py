"""GPU: the trajectory-descriptor kernel (csrc/features.hip, ops.trajectory_features) against the reference goldens, against
the host build of the same header on 2 000 seeded walks, over dtypes and batch sizes; permutation invariance; the batch
entry on CUDA tensors; and a reduced ImagesFeatures run with feature_device="cuda" against the CPU run.  No scipy here."""
import numpy as np
import pytest
import torch

from trajfeat_common import GOLDEN, check_against, golden_ok, host_features, max_sq, rel_err, walks

pytestmark = pytest.mark.gpu


def _kernel(tr, npos=1, dt=1.0, with_average=False):
    from moleculardiffusion_mivit_amd import ops
    r = ops.trajectory_features(torch.as_tensor(np.ascontiguousarray(tr)).cuda(), npos, dt, return_average=with_average)
    torch.cuda.synchronize()
    return (r[0].cpu().numpy(), r[1].cpu().numpy()) if with_average else r.cpu().numpy()


def test_kernel_matches_reference_goldens():
    fx = np.load(GOLDEN)
    for i in range(int(fx["n"])):
        got = _kernel(np.asarray(fx[f"traj{i}"], dtype=np.float64)[None])[0]
        e = rel_err(got, fx[f"feat{i}"])
        assert golden_ok(e), (i, int(np.argmax(e)), e.max())


def test_kernel_matches_host_on_seeded_walks():
    W = walks()
    got, ref = [], []
    for n in sorted({len(w) for w in W}):                 # one launch per length
        batch = np.stack([w for w in W if len(w) == n])
        got.append(_kernel(batch))
        ref.append(host_features(batch))
    got, ref = np.concatenate(got), np.concatenate(ref)
    order = [w for n in sorted({len(w) for w in W}) for w in W if len(w) == n]
    msgs = check_against(got, ref, np.array([max(max_sq(w), 1e-300) for w in order]), [len(w) for w in order])
    assert not msgs, msgs


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [0, 1, 320, 100_000])
def test_dtypes_and_batch_sizes(dtype, n):
    rng = np.random.default_rng(n)
    tr = (np.cumsum(rng.normal(size=(n, 300, 2)), axis=1) / 100).astype(dtype)
    got, avg = _kernel(tr, npos=10, with_average=True)
    assert got.shape == (n, 25) and got.dtype == np.float64 and avg.shape == (n, 30, 2) and avg.dtype == dtype
    if n == 0:
        return
    sel = np.unique(np.linspace(0, n - 1, min(n, 400)).astype(int))          # host reference on a spread sample
    ref, ref_avg = host_features(tr[sel], npos=10, with_average=True)
    assert np.array_equal(avg[sel], ref_avg)                                  # averaging in the input precision, bitwise
    msgs = check_against(got[sel], ref, np.array([max(max_sq(a), 1e-300) for a in ref_avg.astype(np.float64)]),
                         [30] * len(sel))
    assert not msgs, msgs


def test_permuted_batch_gives_permuted_rows_bitwise():
    tr = np.cumsum(np.random.default_rng(7).normal(size=(500, 300, 2)), axis=1) / 100
    perm = np.random.default_rng(8).permutation(500)
    a, b = _kernel(tr, npos=10), _kernel(tr[perm], npos=10)
    assert np.array_equal(a[perm], b, equal_nan=True)


def test_batch_entry_on_cuda_tensors():
    from moleculardiffusion_mivit_amd.helpers import features as ft
    tr = np.cumsum(np.random.default_rng(4).normal(size=(64, 300, 2)), axis=1) / 100
    got = ft.compute_features_for_multiple_trajectories(torch.as_tensor(tr).cuda(), dt=1, nPosPerFrame=10)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (64, 25)
    ref = np.nan_to_num(host_features(tr, npos=10), nan=0.0)
    assert not check_against(got.cpu().numpy(), ref, np.ones(64), [30] * 64, fit_frac=0.95)
    short = ft.compute_features_for_multiple_trajectories(torch.as_tensor(tr[:, :20]).cuda(), nPosPerFrame=10)
    assert torch.equal(short, torch.zeros_like(short))                       # NaN rows -> 0
    with pytest.raises(ValueError):
        ft.compute_features_for_multiple_trajectories(torch.as_tensor(tr[:, :295]).cuda(), nPosPerFrame=10)


def test_images_features_run_with_gpu_features_matches_cpu_run(monkeypatch, tmp_path):
    from moleculardiffusion_mivit_amd.experiments.ImagesFeatures import trainModelsImagesFeatures as M
    from moleculardiffusion_mivit_amd.experiments.ImagesFeatures import trainSettingsImagesFeatures as S
    orig = S.create_video_and_feature_pairs

    def run(feature_device):
        seen = []

        def spy(*a, **k):
            out = orig(*a, **k)
            seen.append(out)
            return out
        monkeypatch.setattr(S, "create_video_and_feature_pairs", spy)
        models, losses, labels = M.run_training(num_cycles=2, N=4, seed=3, out_dir=str(tmp_path), save=False,
                                                model_filter=[S.ft_mlp, S.im_ft_late_tr], feature_device=feature_device)
        return seen, losses, labels

    cpu, cpu_losses, cpu_labels = run(None)
    gpu, gpu_losses, gpu_labels = run("cuda")
    assert len(cpu) == len(gpu) > 0
    assert np.array_equal(cpu_labels, gpu_labels)
    for (v0, f0, t0), (v1, f1, t1) in zip(cpu, gpu):
        assert np.array_equal(v0, v1)                                          # videos
        for a, b in zip(t0, t1):
            assert np.array_equal(a, b)                                        # trajectories, averaged, noisy
        assert f0.dtype == f1.dtype == np.float32
        # features: float32 of the same fp64 numbers (the fit-free ones) or within the fit bar
        e = rel_err(f1.astype(np.float64), f0.astype(np.float64), floor=1e-6)
        assert (e <= 1e-6).mean() > 0.99, e.max()
    for name in gpu_losses:
        v = np.array(gpu_losses[name]["val_avg"])
        assert np.isfinite(v).all(), name
