"""Classical mean-square-displacement estimate of the diffusion coefficient (reference helpers/helpersMSD.py:27-52
``mean_square_displacements``, :124-143 ``estimateDfromMSDs``, :145-172 ``estimateDfromMSDsWeighted``): what the tracks of a
real movie are compared with.  numpy arrays in, numpy arrays out; torch tensors (CPU or GPU) in, tensors on the same device
out.  No plotting."""
import numpy as np
import torch


def mean_square_displacements(trajectories):
    """trajectories [nparticles, num_steps, 2] -> MSD [nparticles, num_steps]; entry tau is the mean over all start times of
    the squared displacement after tau steps, entry 0 is 0."""
    n, steps, _ = trajectories.shape
    if torch.is_tensor(trajectories):
        msd = torch.zeros(n, steps, dtype=trajectories.dtype if trajectories.is_floating_point() else torch.float64,
                          device=trajectories.device)
        for tau in range(1, steps):
            msd[:, tau] = ((trajectories[:, tau:] - trajectories[:, :steps - tau]) ** 2).sum(dim=2).to(msd.dtype).mean(dim=1)
        return msd
    msd = np.zeros((n, steps))
    for tau in range(1, steps):
        msd[:, tau] = np.mean(np.sum((trajectories[:, tau:] - trajectories[:, :steps - tau]) ** 2, axis=2), axis=1)
    return msd


def estimateDfromMSDs(msds, time_range):
    """Least-squares line through the origin, MSD = 4 D t, for every particle: msds [nparticles, T], time_range [T] ->
    D [nparticles]."""
    if torch.is_tensor(msds):
        t = torch.as_tensor(time_range, dtype=msds.dtype, device=msds.device).reshape(-1, 1)
        return torch.linalg.lstsq(t, msds.T).solution[0] / 4
    slopes = np.linalg.lstsq(np.asarray(time_range).reshape(-1, 1), msds.T, rcond=None)[0][0]
    return slopes / 4


def estimateDfromMSDsWeighted(msds, time_range):
    """D from MSD[tau] / tau averaged with weights T - tau (short lags count more): msds [nparticles, T] -> D [nparticles].
    time_range is not used, as in the reference (the lag is counted in steps)."""
    T = msds.shape[1]
    if torch.is_tensor(msds):
        weights = torch.arange(T, 0, -1, dtype=msds.dtype, device=msds.device)
        lag = torch.arange(0, T, dtype=msds.dtype, device=msds.device)
        lag[0] = 1                                              # MSD[0] = 0, so any divisor does
        return (msds / lag[None, :]) @ weights / weights.sum() / 4
    weights = np.arange(T, 0, -1)
    lag = np.arange(0, T)
    lag[0] = 1
    return (msds / lag[np.newaxis, :]) @ weights / np.sum(weights) / 4
