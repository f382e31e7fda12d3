"""Training loop of the Denoising experiment: drop-in for the reference's
``Experiments/Denoising/trainModels_different_settings.py`` (``load_validation_dataMult`` :13-37, data refresh per cycle
:133-180, per-model epoch :184-210 with every model reading its channel ``images_idx_from_name(name)``, validation on
D = 1, 3, 5, 7 :214-247, save :253-260 to ``training_results_mult_Test.pth``).

    python -m moleculardiffusion_mivit_amd.experiments.Denoising.trainModels_different_settings       # the reference run
    ... run_training(num_cycles=2, N=8, TrainingDs_list=([1, 1], [5, 1]), setting_names=["no_noise", "RL_2"])

Every video is (N, 7, 30, 9, 9): the four settings of ``trajectories_to_video_multiple_settings`` and the RL-TV snapshots
after iterations 2, 5 and 10 (``helpers/generation.trajs_to_vid_norm_rl``).  Data is generated on the training device: on
the GPU the renderer, the Gaussian filter and the RL-TV deconvolution are HIP kernels (csrc/render.hip, csrc/deconv.hip).
"""
import numpy as np
import torch

from ...helpers import generation as gen
from .. import _common as C
from . import trainSettingsMult as S
from .trainSettingsMult import *           # noqa: F401,F403  (constants + factories, as the reference does :7)

VAL_D_VALUES = (1, 3, 5, 7)
RESULTS_NAME = "mult_Test"


def load_validation_dataMult(rl_iterations, length=30, generator=None, device="cpu"):
    """(vid1, vid3, vid5, vid7): the fixed validation sets (reference val{1,3,5,7}.npy of this length when
    MIVIT_VALIDATION_ROOT / ../validation_trajectories exists, seeded Brownian otherwise) through trajs_to_vid_norm_rl.
    `generator` drives the trajectories (CPU), the renderer's noise draws a generator on `device` seeded from it."""
    if length not in (20, 30):
        raise ValueError(f"Invalid length value, select one in: {[20, 30]}")
    g = generator or torch.Generator().manual_seed(20250815)
    sets, _ = C.validation_trajectories(length, S.T, S.traj_div_factor, g, d_values=VAL_D_VALUES)
    gd = _device_generator(g, device)
    return tuple(torch.as_tensor(gen.trajs_to_vid_norm_rl(torch.as_tensor(tr, dtype=torch.float32, device=device),
                                                          S.nPosPerFrame, center=True, image_props=S.image_props,
                                                          rl_iterations=rl_iterations, generator=gd))
                 for tr in sets)


def _device_generator(g, device):
    """A generator on `device` seeded from the CPU generator g (None stays None)."""
    if g is None:
        return None
    return torch.Generator(device=device).manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=g)))


def run_training(num_cycles=10, N=64, TrainingDs_list=([1, 1], [3, 1], [5, 1], [7, 1]), setting_names=None, seed=None,
                 out_dir=".", save=True, device=None, verbose=False, **model_kwargs):
    """setting_names: train only the models of these settings (default: all seven, 14 models)."""
    device = torch.device(device or S.device)
    g = torch.Generator().manual_seed(seed) if seed is not None else None
    gd = _device_generator(g, device)
    models, optimizers, schedulers = S.getModels(**model_kwargs)
    if setting_names is not None:
        keep = {f(s) for s in setting_names for f in (S.t_name, S.r_name)}
        unknown = set(setting_names) - set(S.settings)
        if unknown:
            raise ValueError(f"unknown settings {sorted(unknown)}, choose from {S.settings}")
        models = {k: v for k, v in models.items() if k in keep}
    val_videos = load_validation_dataMult(S.RL_iterations, S.nFrames, generator=g, device=device)
    val_sets = [((v,), D) for v, D in zip(val_videos, VAL_D_VALUES)]

    def make_batch_data(cycle):
        vids, labs = [], []
        for Ds in TrainingDs_list:
            trajs, labels = gen.brownian_single_state(N, S.T, Ds=Ds, alphas=1, generator=gd, device=device)
            labs.append(labels[0, :, 1].cpu().numpy())
            vids.append(torch.as_tensor(gen.trajs_to_vid_norm_rl(trajs.permute(1, 0, 2) / S.traj_div_factor, S.nPosPerFrame,
                                                                 S.center, S.image_props, S.RL_iterations, generator=gd)))
        raw = np.concatenate(labs)
        return torch.cat(vids), torch.tensor(raw / S.D_max_normalization, dtype=torch.float32).unsqueeze(-1), raw

    def predict(model, name, images):
        return model(images[:, S.images_idx_from_name(name)])

    models, validation_losses, all_gen_labels = C.run_cycles(
        S, models, optimizers, schedulers, make_batch_data, predict, num_cycles, val_sets, RESULTS_NAME, device=device,
        out_dir=out_dir, save=False, generator=g, verbose=verbose, d_values=VAL_D_VALUES)
    print(f"Number of generated sequences: {all_gen_labels.shape}")
    if save and C.DataParallel().rank == 0:
        C.save_results(validation_losses, all_gen_labels, models, RESULTS_NAME, "", out_dir)
    return models, validation_losses, all_gen_labels


if __name__ == "__main__":
    run_training()
