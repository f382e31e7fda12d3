"""Classical mean-square-displacement estimate of the diffusion coefficient (reference helpers/helpersMSD.py:27-52
``mean_square_displacements``, :124-143 ``estimateDfromMSDs``, :145-172 ``estimateDfromMSDsWeighted``): what the tracks of a
real movie are compared with.  numpy arrays in, numpy arrays out; torch tensors (CPU or GPU) in, tensors on the same device
out.  No plotting.  The ragged tracks of a movie go to track_msd (one launch of csrc/diffusion.hip for CUDA tensors); the
single-track functions of the reference (:7-26 ``mean_square_displacement``, :90-107 ``estimateDfromMSD``) are here too."""
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


def estimate_alpha(msds, max_lag=None):
    """Anomalous exponent of every track: the least-squares slope of log MSD against log lag over the lags 1 .. max_lag
    (default: all) of msds [n_tracks, Lmax], the rows track_msd returns (entry 0 is lag 0 and not used) -> alpha [n_tracks].
    Lags whose MSD is not positive are skipped (the zero padding of a short track's row, a track that did not move); a
    track with fewer than two usable lags gets NaN.  Plain torch ops on the input's device; numpy in, numpy out."""
    is_t = torch.is_tensor(msds)
    m = msds if is_t else torch.as_tensor(np.asarray(msds))
    if m.dim() != 2:
        raise ValueError(f"msds must be [n_tracks, Lmax], got {tuple(m.shape)}")
    M = m.shape[1] - 1
    if max_lag is not None:
        if int(max_lag) != max_lag or max_lag < 1:
            raise ValueError(f"max_lag must be None or an integer >= 1, got {max_lag}")
        M = min(M, int(max_lag))
    m = m[:, 1:M + 1].double()
    ok = m > 0                                                  # NaN is not usable either
    w = ok.double()
    x = torch.log(torch.arange(1, M + 1, dtype=torch.float64, device=m.device)).view(1, -1)
    y = torch.log(torch.where(ok, m, torch.ones((), dtype=torch.float64, device=m.device)))
    cnt = w.sum(dim=1, keepdim=True)
    xm, ym = (w * x).sum(dim=1, keepdim=True) / cnt, (w * y).sum(dim=1, keepdim=True) / cnt
    dx = w * (x - xm)
    alpha = (dx * (y - ym)).sum(dim=1) / (dx * (x - xm)).sum(dim=1)
    alpha = torch.where(cnt.view(-1) >= 2, alpha, torch.full((), float("nan"), dtype=torch.float64, device=m.device))
    return alpha if is_t else alpha.numpy()


def mean_square_displacement(traj):
    """Reference mean_square_displacement (helpers/helpersMSD.py:7-26): one trajectory [num_steps, 2] -> MSD [num_steps]."""
    traj = np.asarray(traj)
    steps = traj.shape[0]
    msd = np.zeros(steps)
    for tau in range(1, steps):
        msd[tau] = np.mean(np.sum((traj[tau:] - traj[:steps - tau]) ** 2, axis=1))
    return msd


def estimateDfromMSD(msd, time_range):
    """Reference estimateDfromMSD (helpers/helpersMSD.py:90-107): least-squares line through the origin for one MSD curve [T]
    -> D (a float)."""
    slope, = np.linalg.lstsq(np.asarray(time_range).reshape(-1, 1), np.asarray(msd), rcond=None)[0]
    return slope / 4


def _check_offsets(offsets, n):
    """CSR offsets [n_tracks + 1] over n rows, array or tensor: the two ends and the monotony, checked on the input's device."""
    if len(offsets.shape) != 1 or offsets.shape[0] < 1:
        raise ValueError(f"offsets must be [n_tracks + 1], got {tuple(offsets.shape)}")
    if int(offsets[0]) != 0 or int(offsets[-1]) != n:
        raise ValueError(f"offsets must start at 0 and end at the number of rows {n}, got {int(offsets[0])} .. {int(offsets[-1])}")
    if offsets.shape[0] > 1 and bool((offsets[1:] < offsets[:-1]).any()):
        raise ValueError("offsets must not decrease")


def _track_msd_numpy(pos, offsets, dt, max_lag):
    """The arithmetic of csrc/diffusion.hip::df_msd_kernel in its order: np.cumsum(...)[-1] is a sequential sum."""
    n_tracks = len(offsets) - 1
    lengths = np.diff(offsets)
    Lmax = int(lengths.max()) if n_tracks else 0
    msd = np.zeros((n_tracks, Lmax))
    d_lstsq, d_weighted = np.full(n_tracks, np.nan), np.full(n_tracks, np.nan)
    for k in range(n_tracks):
        p = pos[offsets[k]:offsets[k + 1]]
        L = len(p)
        M = L - 1 if max_lag == 0 else min(L - 1, max_lag)
        if M < 1:
            continue
        for tau in range(1, M + 1):
            dy, dx = p[tau:, 0] - p[:L - tau, 0], p[tau:, 1] - p[:L - tau, 1]
            msd[k, tau] = np.cumsum(dy * dy + dx * dx)[-1] / float(L - tau)
        lag = np.arange(1, M + 1, dtype=np.float64)
        t, m = lag * dt, msd[k, 1:M + 1]
        d_lstsq[k] = np.cumsum(t * m)[-1] / np.cumsum(t * t)[-1] / 4.0
        d_weighted[k] = np.cumsum((m / lag) * (float(M + 1) - lag))[-1] / (float(M + 1) * float(M + 2) / 2.0) / 4.0
    return msd, d_lstsq, d_weighted


def track_msd(positions, offsets, dt=1.0, max_lag=None):
    """MSD and both classical estimates of D for ragged tracks: positions [N, 2] (y, x) sorted by track and by frame within a
    track, offsets [n_tracks + 1] in CSR form (from 0 to N) -> (msd [n_tracks, Lmax], d_lstsq [n_tracks], d_weighted
    [n_tracks]), float64, Lmax the longest track.  CUDA tensors go to the kernel (ops.track_msd, one launch), numpy arrays and
    CPU tensors to its numpy restatement, bitwise equal; the output is of the input's kind.

    A lag is counted in ROWS.  Tracks from this package's frame-to-frame linking have no gaps (a track that is not linked in a
    frame ends), and the tables of gap closing (max_gap > 0) are FILLED: tracking.fill_gaps adds a row for every missed frame,
    so a lag in rows is a lag in frames.  A table that is gap-closed but not filled must not be passed, and tracks from
    elsewhere must be gap-free too.  Per track of L rows, with M = L - 1 or
    min(L - 1, max_lag), all sums in ascending index:
        msd[tau]   = (sum_i (dy * dy + dx * dx)) / (L - tau), tau = 1 .. M; entry 0 and the entries past M are 0
        d_lstsq    = (sum_tau (tau dt) msd[tau]) / (sum_tau (tau dt)^2) / 4     estimateDfromMSDs: a line through the origin
        d_weighted = (sum_tau (msd[tau] / tau) (M + 1 - tau)) / ((M + 1)(M + 2) / 2) / 4
    d_weighted is estimateDfromMSDsWeighted with T = M + 1: its weight sum includes the weight M + 1 of lag 0, whose term is
    0, and the lag is counted in steps, not in times (dt does not enter), as in the reference.  A track with M < 1 gets a zero
    row and NaN for both estimates."""
    max_lag = 0 if max_lag is None else max_lag
    if int(max_lag) != max_lag or max_lag < 0:
        raise ValueError(f"max_lag must be None or an integer >= 0 (0: all lags), got {max_lag}")
    if len(positions.shape) != 2 or positions.shape[1] != 2:
        raise ValueError(f"positions must be [N, 2], got {tuple(positions.shape)}")
    if torch.is_tensor(positions) != torch.is_tensor(offsets):
        raise ValueError("positions and offsets must both be tensors or both be arrays")
    if torch.is_tensor(positions) and positions.device != offsets.device:
        raise ValueError(f"positions on {positions.device}, offsets on {offsets.device}")
    offsets = offsets if torch.is_tensor(offsets) else np.asarray(offsets)
    _check_offsets(offsets, positions.shape[0])
    if torch.is_tensor(positions) and positions.device.type == "cuda":
        from .. import ops
        return ops.track_msd(positions.double(), offsets.int(), float(dt), int(max_lag))
    if torch.is_tensor(positions):
        out = _track_msd_numpy(positions.detach().double().numpy(), offsets.detach().numpy().astype(np.int64), float(dt),
                               int(max_lag))
        return tuple(torch.from_numpy(a) for a in out)
    return _track_msd_numpy(np.asarray(positions, dtype=np.float64), offsets.astype(np.int64), float(dt), int(max_lag))
