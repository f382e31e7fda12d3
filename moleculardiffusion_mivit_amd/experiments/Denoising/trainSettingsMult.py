"""Denoising experiment settings: drop-in for the reference's ``Experiments/Denoising/trainSettingsMult.py`` (constants
:13-86, ``settings`` / ``RL_iterations`` :90-94, ``r_name`` / ``t_name`` / ``images_idx_from_name`` :97-116, ``getModels``
:125-159): one DeepResNet transformer and one MultiImageResNet per image setting -- no noise, Gaussian background, Poisson
noise, Gaussian-filtered Poisson, and RL-TV deconvolution of the Poisson video stopped after iterations 2, 5 and 10.

Addition the reference does not have (optional, the default reproduces the reference): ``getModels(precision=)``.
The sequence-prediction branch (``sequences = True``), which the reference never runs, is not mirrored."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

from ...helpers.models import *            # noqa: F401,F403  (same star-import surface as the reference :4)
from ...helpers.models import DeepResNetEmbedding, GeneralTransformer, MLPHead, MultiImageResNet

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

sequences = False
center = True
adaptive_batch_size = 20          # batch size doubles every `adaptive_batch_size` cycles (-1: fixed)
lr = 1e-4
D_max_normalization = 10

loss_function = nn.L1Loss()
val_loss_function = nn.L1Loss(reduction='none')
single_prediction = True
use_regression_token = True
use_pos_encoding = True
tr_activation_fct = F.relu

patch_size = 9
embed_dim = 64
num_heads = 4
hidden_dim = 128
num_layers = 6
dropout = 0.0

traj_div_factor = 100             # trajectories are given in pixels/s, wanted in the ms domain
nPosPerFrame = 10
nFrames = 30                      # sequence length
T = nFrames * nPosPerFrame
background_mean, background_sigma = 1420, 290
part_mean, part_std = 5400 - background_mean, 500

image_props = {
    "particle_intensity": [part_mean, part_std],
    "NA": 1.46,
    "wavelength": 500e-9,
    "psf_division_factor": 1.3,
    "resolution": 100e-9,
    "output_size": patch_size,
    "upsampling_factor": 5,
    "background_intensity": [background_mean, background_sigma],
    "poisson_noise": 100,
    "trajectory_unit": 1200,
}

RL_iterations = [2, 5, 10]
settings = ["no_noise", "gaussian_noise", "poisson_noise", "gauss_filter"] + ["RL_" + str(rl) for rl in RL_iterations]


def r_name(setting):
    return "resnet_" + setting


def t_name(setting):
    return "trans_" + setting


def images_idx_from_name(name):
    """Channel of trajs_to_vid_norm_rl's output a model trains on; -1 for an unknown name."""
    for idx, key in enumerate(("no_noise", "gaussian_noise", "poisson_noise", "gauss_filter")):
        if key in name:
            return idx
    if "RL" in name:
        return 4 + RL_iterations.index(int(name.split("_")[-1]))
    return -1


val_d_in_order = np.arange(0.1, 7.01, 0.1)
N_in_order = 10

embed_kwargs = {"patch_size": patch_size, "embed_dim": embed_dim}
twoLayerMLP = MLPHead


def getModels(precision=None):
    """{'trans_<setting>': MiViT with a DeepResNet embedding, 'resnet_<setting>': MultiImageResNet} for the 7 settings, each
    with AdamW(lr) and StepLR(5, 0.9)."""
    models, optimizers, schedulers = {}, {}, {}
    for setting in settings:
        trans = GeneralTransformer(embedding_cls=DeepResNetEmbedding, embed_kwargs=embed_kwargs, embed_dim=embed_dim,
                                   num_heads=num_heads, hidden_dim=hidden_dim, num_layers=num_layers, mlp_head=twoLayerMLP,
                                   tr_activation_fct=tr_activation_fct, dropout=dropout, use_pos_encoding=use_pos_encoding,
                                   use_regression_token=use_regression_token, single_prediction=single_prediction,
                                   precision=precision)
        resnet = MultiImageResNet(patch_size, single_prediction=single_prediction, activation=nn.ReLU)
        for name, model in ((t_name(setting), trans), (r_name(setting), resnet)):
            opt = optim.AdamW(model.parameters(), lr=lr)
            models[name] = model
            optimizers[name] = opt
            schedulers[name] = optim.lr_scheduler.StepLR(opt, step_size=5, gamma=0.9)
    return models, optimizers, schedulers
