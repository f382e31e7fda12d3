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


# ----------------------------------------------------------------------------------------------------------------------
# multi-state tracks: changepoints of the step variance and one row of estimates per segment (csrc/segment.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _segment_numpy(pos, offsets, min_len, penalty, min_var, return_margin=False):
    """The arithmetic of csrc/segment.hip::partition_kernel<VarianceModel> in its order (include/mivit_hip.h, mivit_segment_tracks):
    np.cumsum is the sequential prefix sum, np.argmin returns the lowest index among equal minima.  pos [N, 2] float64,
    offsets [n_tracks + 1] int64 -> (seg_start [N] int32, cost [n_tracks] float64).  Differs from the kernel in log alone.
    return_margin: also margin [n_tracks], the smallest gap between the chosen candidate and the runner-up over the steps j
    on the backtracked path (inf where no such step had two candidates): how far rounding is from changing the partition."""
    n_tracks = len(offsets) - 1
    seg_start = np.zeros(len(pos), np.int32)
    cost = np.full(n_tracks, np.nan)
    margin = np.full(n_tracks, np.inf)
    for k in range(n_tracks):
        a, b = int(offsets[k]), int(offsets[k + 1])
        L = b - a
        if L >= 1:
            seg_start[a] = 1
        Linc = L - 1
        if Linc < 1:
            continue
        p = pos[a:b]
        dy, dx = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
        cs = np.concatenate([np.zeros(1), np.cumsum(dy * dy + dx * dx)])
        beta = penalty * np.log(float(Linc))

        def step(j, cand):
            tn = 2.0 * (j - cand).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                return (F[cand] + tn * np.log(np.maximum((cs[j] - cs[cand]) / tn, min_var))) + beta

        F = np.full(Linc + 1, np.nan)
        F[0] = -beta
        if Linc < min_len:
            cost[k] = step(Linc, np.zeros(1, np.int64))[0]
            continue
        prev = np.zeros(Linc + 1, np.int64)
        gap = np.full(Linc + 1, np.inf)
        for j in range(min_len, Linc + 1):
            cand = np.concatenate([np.zeros(1, np.int64), np.arange(min_len, j - min_len + 1, dtype=np.int64)])
            v = step(j, cand)
            m = int(np.argmin(v)) if not np.isnan(v).all() else 0
            F[j], prev[j] = v[m], cand[m]
            if return_margin and len(v) > 1:
                gap[j] = np.partition(v, 1)[1] - v[m]
        cost[k] = F[Linc]
        j = Linc
        while j > 0:
            margin[k] = min(margin[k], gap[j])
            i = int(prev[j])
            if i > 0:
                seg_start[a + i] = 1
            j = i
    return (seg_start, cost, margin) if return_margin else (seg_start, cost)


def _segment_stats_numpy(pos, seg_offsets, seg_track_end, dt, blur):
    """The arithmetic of csrc/segment.hip::stretch_stats_kernel<false> in its order: np.cumsum(...)[-1] is a sequential sum.  -> (D_cve,
    D_mle, sigma2 [n_seg] float64, n_increments [n_seg] int32), bitwise the kernel's."""
    n_seg = len(seg_track_end)
    d_cve, d_mle, sigma2 = np.full(n_seg, np.nan), np.full(n_seg, np.nan), np.full(n_seg, np.nan)
    n_inc = np.zeros(n_seg, np.int32)
    R = float(blur)
    for s in range(n_seg):
        r0 = int(seg_offsets[s])
        r1 = min(int(seg_offsets[s + 1]), int(seg_track_end[s]) - 1, len(pos) - 1)
        n = max(r1 - r0, 0)
        n_inc[s] = n
        if n < 1:
            continue
        p = pos[r0:r1 + 1]
        dy, dx = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
        S2 = np.cumsum(dy * dy + dx * dx)[-1]
        d_mle[s] = S2 / ((4.0 * float(n)) * dt)
        if n >= 2:
            S11 = np.cumsum(dy[:-1] * dy[1:] + dx[:-1] * dx[1:])[-1]
            m1 = 2.0 * float(n - 1)
            d_cve[s] = d_mle[s] + S11 / (m1 * dt)
            sigma2[s] = (R * S2) / (2.0 * float(n)) + ((2.0 * R - 1.0) * S11) / m1
    return d_cve, d_mle, sigma2, n_inc


def _check_partition_args(positions, offsets, dt, min_len, penalty, min_var, blur, limit_name):
    """What segment_tracks and segment_transport check alike -> offsets (a tensor as it came, anything else as an array).
    limit_name: the caller's name for ops.SEG_MAX_LEN, for the message."""
    if isinstance(min_len, bool) or int(min_len) != min_len or min_len < 2:
        raise ValueError(f"min_len must be an integer >= 2, got {min_len}")
    if not float(penalty) >= 0.0:
        raise ValueError(f"penalty must be >= 0, got {penalty}")
    if not 0.0 < float(min_var) < float("inf"):
        raise ValueError(f"min_var must be positive and finite, got {min_var}")
    if not 0.0 < float(dt) < float("inf"):
        raise ValueError(f"dt must be positive and finite, got {dt}")
    if not 0.0 <= float(blur) <= 0.25:
        raise ValueError(f"blur must lie in [0, 1/4], got {blur}")
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
        lengths = offsets[1:] - offsets[:-1]
        if len(lengths) and int(lengths.max()) > ops.SEG_MAX_LEN:
            raise ValueError(f"a track of {int(lengths.max())} rows on the GPU, the kernel's limit is {ops.SEG_MAX_LEN} "
                             f"(ops.{limit_name})")
    return offsets


def _stretch_layout(seg_start, offsets, n_rows):
    """seg_start [N] (1 on the first row of every stretch) and offsets [n_tracks + 1] int64, both tensors or both arrays ->
    (first [n_seg] int64, the first row of every stretch; seg_offsets [n_seg + 1] int64, their CSR over the rows; seg_track
    [n_seg] int64; track_end [n_seg] int64, the row at which each stretch's track ends)."""
    if torch.is_tensor(seg_start):
        first = torch.nonzero(seg_start, as_tuple=True)[0]
        seg_offsets = torch.cat([first, torch.full((1,), n_rows, dtype=torch.int64, device=first.device)])
        seg_track = torch.searchsorted(offsets, first, right=True) - 1
    else:
        first = np.nonzero(seg_start)[0].astype(np.int64)
        seg_offsets = np.concatenate([first, np.full(1, n_rows, np.int64)])
        seg_track = np.searchsorted(offsets, first, side="right").astype(np.int64) - 1
    # an empty track shares its offset with the next one: the LAST track that starts at or before the row owns it
    return first, seg_offsets, seg_track, offsets[seg_track + 1]


def segment_tracks(positions, offsets, dt=1.0, min_len=4, penalty=3.0, min_var=1e-12, blur=0.0):
    """Tracks whose diffusion coefficient changes: the optimal partition of every track into stretches of constant step
    variance, and the estimates of each stretch.  positions [N, 2] (y, x) sorted by track and by frame, offsets [n_tracks + 1]
    (CSR), as track_msd takes them (gap-free rows) -> dict:
        seg_offsets [n_seg + 1] int64   CSR of the segments over the same rows: track_msd, tracking.plan_sequences and
                                        tracking.track_sequences accept it in place of offsets
        seg_track   [n_seg] int64       the track of each segment
        D_cve, D_mle, sigma2 [n_seg] float64, n_increments [n_seg] int64
        cost        [n_tracks] float64  the penalised cost of the partition, NaN for a track without an increment
    Penalised likelihood (optimal partitioning): the increments of a stretch are Gaussian with one variance, a stretch has at
    least min_len increments, and every changepoint costs beta = penalty * log(increments of the track); a variance below
    min_var counts as min_var (a track that does not move).  The changepoint at increment c puts row c into the later
    segment; the increment that bridges two segments is counted in the earlier one's estimates.  D_mle = <q> / (4 dt) is the
    maximum-likelihood estimate without localisation noise, which adds sigma^2 / dt to it; D_cve (Vestergaard et al. 2014)
    adds the covariance of neighbouring increments, in which localisation noise and motion blur cancel, and sigma2 is the
    localisation variance that goes with it, with blur the motion-blur coefficient R (0: instantaneous exposure, 1/6: the
    whole frame).  D_cve and sigma2 are NaN for a segment of fewer than 2 increments.  include/mivit_hip.h has the
    arithmetic.  CUDA tensors go to the kernels (csrc/segment.hip: two launches; a track has at most ops.SEG_MAX_LEN rows),
    numpy arrays and CPU tensors to the numpy restatements; the output is of the input's kind."""
    offsets = _check_partition_args(positions, offsets, dt, min_len, penalty, min_var, blur, "SEG_MAX_LEN")
    min_len, penalty, min_var, dt, blur = int(min_len), float(penalty), float(min_var), float(dt), float(blur)
    is_t = torch.is_tensor(positions)
    if is_t and positions.device.type == "cuda":
        from .. import ops
        pos = positions.detach().double().contiguous()
        seg_start, cost = ops.segment_tracks(pos, offsets.int().contiguous(), min_len, penalty, min_var)
        _, seg_offsets, seg_track, track_end = _stretch_layout(seg_start, offsets.long().contiguous(), pos.shape[0])
        d_cve, d_mle, sigma2, n_inc = ops.segment_stats(pos, seg_offsets.int(), track_end.int(), dt, blur)
        return {"seg_offsets": seg_offsets, "seg_track": seg_track, "D_cve": d_cve, "D_mle": d_mle, "sigma2": sigma2,
                "n_increments": n_inc.long(), "cost": cost}
    pos = positions.detach().double().numpy() if is_t else np.asarray(positions, dtype=np.float64)
    off = (offsets.detach().numpy() if is_t else offsets).astype(np.int64)
    seg_start, cost = _segment_numpy(pos, off, min_len, penalty, min_var)
    _, seg_offsets, seg_track, track_end = _stretch_layout(seg_start, off, len(pos))
    d_cve, d_mle, sigma2, n_inc = _segment_stats_numpy(pos, seg_offsets, track_end, dt, blur)
    out = {"seg_offsets": seg_offsets, "seg_track": seg_track, "D_cve": d_cve, "D_mle": d_mle, "sigma2": sigma2,
           "n_increments": n_inc.astype(np.int64), "cost": cost}
    return {k: torch.from_numpy(v) for k, v in out.items()} if is_t else out


# ----------------------------------------------------------------------------------------------------------------------
# diffusion states shared across tracks: a hidden Markov model over the increments of all tracks (csrc/hmm.hip)
# ----------------------------------------------------------------------------------------------------------------------
_LOG_2PI = float(np.log(2.0 * np.pi))


def _hmm_layout(pos, offsets):
    """What both restatements share: the first row a and the increments T of every track, the tracks in descending T (so the
    tracks still running at step t are a prefix), and q of every row (the increment to the next row, track ends included:
    those are never read)."""
    a = offsets[:-1].astype(np.int64)
    T = np.diff(offsets).astype(np.int64) - 1
    order = np.argsort(-T, kind="stable")
    Ts = T[order]
    with np.errstate(over="ignore", invalid="ignore"):
        dy, dx = pos[1:, 0] - pos[:-1, 0], pos[1:, 1] - pos[:-1, 1]
        q = np.concatenate([dy * dy + dx * dx, np.zeros(1)])
    return a[order], Ts, order, q


def _hmm_estep_numpy(pos, offsets, v, A, pi):
    """The arithmetic of csrc/hmm.hip::hmm_estep_kernel in its order (include/mivit_hip.h, mivit_hmm_estep): every sum over a
    state index is an explicit loop in ascending index that starts at 0, the statistics are summed in descending t.  All
    tracks advance together, one step t at a time (elementwise, so each track's numbers are those of the kernel's lanes).
    pos [N, 2] float64, offsets [n_tracks + 1] int64, v [K], A [K, K], pi [K] -> (gamma [N, K], state [N] int32, xi [n_tracks,
    K, K], g_sum, gq_sum, g_first [n_tracks, K], loglik [n_tracks]).  Differs from the kernel in exp and log alone."""
    n_tracks, K, n_rows = len(offsets) - 1, len(v), len(pos)
    a, Ts, order, q_all = _hmm_layout(pos, offsets)
    gamma, ws = np.full((n_rows, K), np.nan), np.zeros((n_rows, K))
    state = np.full(n_rows, -1, np.int32)
    xi = np.zeros((n_tracks, K, K))
    gs, gqs, gfirst = np.zeros((n_tracks, K)), np.zeros((n_tracks, K)), np.zeros((n_tracks, K))
    slc, sm = np.zeros(n_tracks), np.zeros(n_tracks)
    dead, cbad = np.zeros(n_tracks, bool), np.ones(n_tracks)
    alpha = np.zeros((n_tracks, K))
    vmax = v[0]
    for i in range(1, K):
        vmax = v[i] if v[i] > vmax else vmax
    tvmax, tv = 2.0 * vmax, 2.0 * v
    Tmax = int(Ts[0]) if n_tracks else 0
    nact = [int(np.searchsorted(-Ts, -t, side="left")) for t in range(Tmax + 1)]          # tracks with T > t
    with np.errstate(all="ignore"):
        for t in range(Tmax):
            n = nact[t]
            rows = a[:n] + t
            q = q_all[rows]
            m = q / tvmax
            b = np.exp(-(q[:, None] / tv[None, :] - m[:, None])) / v[None, :]
            if t == 0:
                x = pi[None, :] * b
            else:
                s = np.zeros((n, K))
                for i in range(K):
                    s = s + alpha[:n, i:i + 1] * A[i][None, :]
                x = s * b
            c = np.zeros(n)
            for j in range(K):
                c = c + x[:, j]
            bad = ~((c > 0.0) & (c < np.inf))
            new = bad & ~dead[:n]
            cbad[:n][new] = c[new]
            dead[:n] |= bad
            alpha[:n] = x / c[:, None]
            slc[:n] = slc[:n] + np.log(c)
            sm[:n] = sm[:n] + m
            gamma[rows] = alpha[:n]
            ws[rows] = b / c[:, None]
        beta = np.ones((n_tracks, K))
        for t in range(Tmax - 1, -1, -1):
            n, n2 = nact[t], nact[t + 1]                                                   # n2: the tracks with t < T - 1
            rows = a[:n] + t
            al = gamma[rows]
            if n2:
                w = ws[rows[:n2] + 1] * beta[:n2]
                nb = np.zeros((n2, K))
                for i in range(K):
                    nb = nb + A[:, i][None, :] * w[:, i:i + 1]
                    xi[:n2, i, :] = xi[:n2, i, :] + (al[:n2, i:i + 1] * A[i][None, :]) * w
                beta[:n2] = nb
            gam = al * beta[:n]
            gs[:n] = gs[:n] + gam
            gqs[:n] = gqs[:n] + gam * q_all[rows][:, None]
            bg, best = gam[:, 0].copy(), np.zeros(n, np.int32)
            for i in range(1, K):
                up = gam[:, i] > bg
                bg = np.where(up, gam[:, i], bg)
                best = np.where(up, np.int32(i), best)
            gamma[rows] = gam
            state[rows] = best
            gamma[rows[n2:] + 1] = gam[n2:]                                                # the last row repeats
            state[rows[n2:] + 1] = best[n2:]
            if t == 0:
                gfirst[:n] = gam
        loglik = (slc - sm) - Ts.astype(np.float64) * _LOG_2PI
    none = Ts < 1
    for arr in (xi, gs, gqs, gfirst, loglik):
        arr[none | dead] = np.nan
    loglik[dead & (cbad == 0.0)] = -np.inf
    for k in np.nonzero(dead)[0]:
        gamma[a[k]:a[k] + Ts[k] + 1] = np.nan
        state[a[k]:a[k] + Ts[k] + 1] = -1
    inv = np.empty(n_tracks, np.int64)
    inv[order] = np.arange(n_tracks)
    return gamma, state, xi[inv], gs[inv], gqs[inv], gfirst[inv], loglik[inv]


def _hmm_viterbi_numpy(pos, offsets, v, logv, logA, logpi):
    """The arithmetic of csrc/hmm.hip::hmm_viterbi_kernel in its order (mivit_hmm_viterbi): a candidate replaces the running
    maximum only where it compares greater, in ascending index, so the lowest index wins among equal maxima and a NaN never
    does (np.argmax would pick it).  The logarithms are inputs.  -> (state [N] int32, logp [n_tracks]), bitwise the kernel's."""
    n_tracks, K, n_rows = len(offsets) - 1, len(v), len(pos)
    a, Ts, order, q_all = _hmm_layout(pos, offsets)
    state = np.full(n_rows, -1, np.int32)
    logp = np.full(n_tracks, np.nan)
    bp = np.zeros((n_rows, K), np.int32)
    end = np.zeros(n_tracks, np.int32)
    delta = np.zeros((n_tracks, K))
    tv = 2.0 * v
    Tmax = int(Ts[0]) if n_tracks else 0
    nact = [int(np.searchsorted(-Ts, -t, side="left")) for t in range(Tmax + 1)]
    with np.errstate(all="ignore"):
        for t in range(Tmax):
            n, n2 = nact[t], nact[t + 1]
            rows = a[:n] + t
            lb = -(q_all[rows][:, None] / tv[None, :]) - logv[None, :]
            if t == 0:
                delta[:n] = logpi[None, :] + lb
            else:
                bv, bi = delta[:n, 0:1] + logA[0][None, :], np.zeros((n, K), np.int32)
                for i in range(1, K):
                    cand = delta[:n, i:i + 1] + logA[i][None, :]
                    up = cand > bv
                    bv = np.where(up, cand, bv)
                    bi = np.where(up, np.int32(i), bi)
                delta[:n] = bv + lb
                bp[rows] = bi
            if n > n2:                                                                     # the tracks that end here
                d = delta[n2:n]
                bv, s = d[:, 0].copy(), np.zeros(n - n2, np.int32)
                for i in range(1, K):
                    up = d[:, i] > bv
                    bv = np.where(up, d[:, i], bv)
                    s = np.where(up, np.int32(i), s)
                logp[n2:n], end[n2:n] = bv, s
        s = end.copy()
        for t in range(Tmax - 1, -1, -1):
            n, n2 = nact[t], nact[t + 1]
            rows = a[:n] + t
            state[rows] = s[:n]
            state[rows[n2:] + 1] = s[n2:n]                                                 # the last row repeats
            if t > 0:
                s[:n] = bp[rows, s[:n]]
    inv = np.empty(n_tracks, np.int64)
    inv[order] = np.arange(n_tracks)
    return state, logp[inv]


def _hmm_inputs(positions, offsets):
    """The checks of track_msd / segment_tracks -> (pos, off, kind): kind "cuda" (float64 / int32 tensors on the GPU), "cpu" or
    "numpy" (float64 / int64 arrays)."""
    if len(positions.shape) != 2 or positions.shape[1] != 2:
        raise ValueError(f"positions must be [N, 2], got {tuple(positions.shape)}")
    if torch.is_tensor(positions) != torch.is_tensor(offsets):
        raise ValueError("positions and offsets must both be tensors or both be arrays")
    if torch.is_tensor(positions) and positions.device != offsets.device:
        raise ValueError(f"positions on {positions.device}, offsets on {offsets.device}")
    offsets = offsets if torch.is_tensor(offsets) else np.asarray(offsets)
    _check_offsets(offsets, positions.shape[0])
    if torch.is_tensor(positions) and positions.device.type == "cuda":
        return positions.detach().double().contiguous(), offsets.int().contiguous(), "cuda"
    if torch.is_tensor(positions):
        return positions.detach().double().numpy(), offsets.detach().numpy().astype(np.int64), "cpu"
    return np.asarray(positions, dtype=np.float64), offsets.astype(np.int64), "numpy"


def _hmm_estep_any(pos, off, kind, v, A, pi):
    """One E-step on the input's device, float64 torch tensors in and out: the kernel on the GPU, the restatement elsewhere."""
    if kind == "cuda":
        from .. import ops
        return ops.hmm_estep(pos, off, v.contiguous(), A.contiguous(), pi.contiguous())
    out = _hmm_estep_numpy(pos, off, v.numpy(), A.numpy(), pi.numpy())
    return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)


def _hmm_viterbi_any(pos, off, kind, v, A, pi):
    if kind == "cuda":
        from .. import ops
        return ops.hmm_viterbi(pos, off, v.contiguous(), A.contiguous(), pi.contiguous())
    with np.errstate(divide="ignore"):
        out = _hmm_viterbi_numpy(pos, off, v.numpy(), np.log(v.numpy()), np.log(A.numpy()), np.log(pi.numpy()))
    return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)


def _hmm_out(d, kind):
    if kind != "numpy":
        return d
    return {k: (x.cpu().numpy() if torch.is_tensor(x) else x) for k, x in d.items()}


def _hmm_scalars(dt, sigma2):
    if not 0.0 < float(dt) < float("inf"):
        raise ValueError(f"dt must be positive and finite, got {dt}")
    if not 0.0 <= float(sigma2) < float("inf"):
        raise ValueError(f"sigma2 must be finite and >= 0, got {sigma2}")
    return float(dt), float(sigma2)


def hmm_posteriors(positions, offsets, Ds, M, p0=None, dt=1.0, sigma2=0.0):
    """The posterior of the hidden state of every row under GIVEN parameters: one E-step and the Viterbi path of the hidden
    Markov model that fit_diffusion_states fits.  positions [N, 2] and offsets [n_tracks + 1] as segment_tracks takes them; Ds
    [K], M [K, K] and p0 [K] as generation.multi_state takes them (p0 = None: the stationary distribution of M) -> dict of the
    input's kind: gamma [N, K], state_posterior [N] (the largest gamma), state [N] (Viterbi), loglik [n_tracks] (the track's
    log-likelihood, -inf where it underflows, NaN without an increment or with a NaN position), logp [n_tracks] (the Viterbi
    path's log-probability up to -T log(2 pi)), and the E-step's statistics xi, g_sum, gq_sum, g_first.  A row holds the
    increment that starts at it; a track's last row repeats the row before it, a one-row track has NaN and -1.  State j has
    the per-axis increment variance 2 Ds[j] dt + 2 sigma2, sigma2 the localisation variance; the correlation that
    localisation noise puts between neighbouring increments is ignored.  include/mivit_hip.h has the arithmetic.  CUDA
    tensors go to the kernels (csrc/hmm.hip, two launches, no limit on a track's length), anything else to the restatements."""
    from .generation import _markov_args
    dt, sigma2 = _hmm_scalars(dt, sigma2)
    Ds, M, p0 = _markov_args(Ds, M, p0)
    pos, off, kind = _hmm_inputs(positions, offsets)
    dev = pos.device if kind == "cuda" else "cpu"
    v = torch.from_numpy(2.0 * Ds * dt + 2.0 * sigma2).to(dev)
    if not bool((v > 0).all()):
        raise ValueError("every state needs a positive increment variance 2 D dt + 2 sigma2")
    A, pi = torch.from_numpy(M).to(dev), torch.from_numpy(p0).to(dev)
    gamma, sp, xi, g_sum, gq_sum, g_first, loglik = _hmm_estep_any(pos, off, kind, v, A, pi)
    state, logp = _hmm_viterbi_any(pos, off, kind, v, A, pi)
    return _hmm_out({"gamma": gamma, "state_posterior": sp.long(), "state": state.long(), "loglik": loglik, "logp": logp,
                     "xi": xi, "g_sum": g_sum, "gq_sum": gq_sum, "g_first": g_first}, kind)


def fit_diffusion_states(positions, offsets, K, dt=1.0, sigma2=0.0, max_iter=200, tol=1e-8, min_var=1e-12, init=None):
    """Diffusion states shared by all tracks of a movie: K diffusion coefficients, their K x K transition probabilities and the
    state of every row, by maximum likelihood (EM) on a hidden Markov model over the increments of ALL tracks -- the inverse
    of generation.multi_state(N, T, Ds, M).  Where segment_tracks cuts each track on its own, this pools: a stretch of a few
    rows is recognised because its state is known from every other track.  positions, offsets as segment_tracks takes them
    (gap-free rows) -> dict of the input's kind, states sorted by ascending D:
        Ds [K], M [K, K], p0 [K]        the fitted parameters (p0: the distribution of a track's first state)
        loglik, n_iter, converged       total log-likelihood of the used tracks, E-steps taken, whether tol was met
        loglik_trace [n_iter]           the log-likelihood of every E-step
        bic                             -2 loglik + (K^2 + K - 1) log(n_increments): compare fits of different K
        n_tracks_used, n_increments     the tracks with a finite log-likelihood and their increments
        gamma [N, K]                    posterior of the state of the increment that starts at each row
        state [N], state_posterior [N]  the Viterbi path under the fitted parameters / the largest gamma; -1 where undefined
        occupancy [K]                   the share of increments in each state
    State j has the per-axis increment variance v_j = 2 D_j dt + 2 sigma2, sigma2 the (given) localisation variance; the
    correlation that localisation noise puts between neighbouring increments is ignored, and D_j = (v_j - 2 sigma2) / (2 dt)
    may come out negative where sigma2 is overstated.  The default start: v at the K quantile mid-points of q / 2 over all
    increments, spread by factors from 0.5 to 2; M with 0.9 on the diagonal and the rest shared equally; p0 uniform.  init = {
    "Ds", "M", "p0"} replaces any of them.  An iteration is an E-step (csrc/hmm.hip on CUDA tensors, its numpy restatement
    elsewhere) and an M-step over the tracks with a finite log-likelihood (a few float64 torch ops on the input's device):
        M[i][j] = Xi[i][j] / sum_j Xi[i][j];  v_j = max(GQ_j / (2 G_j), min_var);  p0 = G_first / sum(G_first)
    (a state nothing was assigned to keeps its row and variance) until loglik - previous < tol * |loglik| or max_iter E-steps;
    only the scalar loglik is read back per iteration.  A track without an increment, with a NaN position or whose likelihood
    underflows contributes nothing."""
    if isinstance(K, bool) or int(K) != K or K < 1:
        raise ValueError(f"K must be an integer >= 1, got {K}")
    K = int(K)
    from .. import ops
    if K > ops.MARKOV_MAX_K:
        raise ValueError(f"K = {K} states, 1 .. {ops.MARKOV_MAX_K} (ops.MARKOV_MAX_K) are supported")
    dt, sigma2 = _hmm_scalars(dt, sigma2)
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, got {max_iter}")
    if not float(tol) >= 0.0:
        raise ValueError(f"tol must be >= 0, got {tol}")
    if not 0.0 < float(min_var) < float("inf"):
        raise ValueError(f"min_var must be positive and finite, got {min_var}")
    init = {} if init is None else dict(init)
    if set(init) - {"Ds", "M", "p0"}:
        raise ValueError(f"init: unknown keys {sorted(set(init) - {'Ds', 'M', 'p0'})}")
    pos, off, kind = _hmm_inputs(positions, offsets)
    dev = pos.device if kind == "cuda" else torch.device("cpu")
    tpos = pos if kind == "cuda" else torch.from_numpy(pos if pos.flags.writeable else pos.copy())
    toff = off.long() if kind == "cuda" else torch.from_numpy(off if off.flags.writeable else off.copy())
    n_rows, n_tracks = tpos.shape[0], toff.numel() - 1
    f64 = dict(dtype=torch.float64, device=dev)
    host = lambda x: np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)    # noqa: E731

    if "Ds" in init:
        d0 = host(init["Ds"]).reshape(-1)
        if d0.shape != (K,) or not np.isfinite(d0).all():
            raise ValueError(f"init['Ds'] must hold {K} finite values")
        v = torch.from_numpy(2.0 * d0 * dt + 2.0 * sigma2).to(dev)
        if not bool((v > 0).all()):
            raise ValueError("init['Ds']: every state needs a positive increment variance 2 D dt + 2 sigma2")
    else:
        # q / 2 of every increment inside a track (E[q] = 2 v), sorted: order statistics, the same on every device
        inside = torch.ones(n_rows, dtype=torch.bool, device=dev)
        inside[toff[1:][toff[1:] > toff[:-1]] - 1] = False
        d = tpos[1:] - tpos[:-1]
        h = ((d * d).sum(dim=1) / 2.0)[inside[:-1]] if n_rows > 1 else torch.zeros(0, **f64)
        h = torch.sort(h[torch.isfinite(h)])[0]
        if h.numel() == 0:
            raise ValueError("no track has a finite increment")
        at = ((torch.arange(K, **f64) + 0.5) / K * h.numel()).long().clamp(max=h.numel() - 1)
        spread = torch.from_numpy(np.geomspace(0.5, 2.0, K) if K > 1 else np.ones(1)).to(dev)
        v = torch.clamp(h[at] * spread, min=float(min_var))
    if "M" in init:
        m0 = host(init["M"])
        if m0.shape != (K, K) or not ((m0 >= 0).all() and np.allclose(m0.sum(axis=1), 1.0, rtol=0, atol=1e-9)):
            raise ValueError(f"init['M'] must be [{K}, {K}] with rows that are distributions")
        A = torch.from_numpy(np.ascontiguousarray(m0)).to(dev)
    else:
        A = torch.full((K, K), 0.1 / (K - 1) if K > 1 else 0.0, **f64)
        A.fill_diagonal_(0.9 if K > 1 else 1.0)
    if "p0" in init:
        q0 = host(init["p0"]).reshape(-1)
        if q0.shape != (K,) or not ((q0 >= 0).all() and abs(q0.sum() - 1.0) <= 1e-9):
            raise ValueError(f"init['p0'] must be a distribution over the {K} states")
        pi = torch.from_numpy(q0).to(dev)
    else:
        pi = torch.full((K,), 1.0 / K, **f64)

    trace, converged, prev = [], False, None
    zero = torch.zeros((), **f64)
    for it in range(int(max_iter)):
        gamma, sp, xi, g_sum, gq_sum, g_first, loglik = _hmm_estep_any(pos, off, kind, v, A, pi)
        ok = torch.isfinite(loglik)
        ll = float(torch.where(ok, loglik, zero).sum())                                    # the one read-back
        trace.append(ll)
        if prev is not None and ll - prev < float(tol) * abs(ll):
            converged = True
            break
        prev = ll
        if it == int(max_iter) - 1:
            break
        Xi = torch.where(ok[:, None, None], xi, zero).sum(dim=0)
        G = torch.where(ok[:, None], g_sum, zero).sum(dim=0)
        GQ = torch.where(ok[:, None], gq_sum, zero).sum(dim=0)
        GF = torch.where(ok[:, None], g_first, zero).sum(dim=0)
        rs = Xi.sum(dim=1, keepdim=True)
        A = torch.where(rs > 0, Xi / rs, A)
        v = torch.where(G > 0, torch.clamp(GQ / (2.0 * G), min=float(min_var)), v)
        pi = torch.where(GF.sum() > 0, GF / GF.sum(), pi)
    Ds = (v - 2.0 * sigma2) / (2.0 * dt)
    perm = torch.argsort(Ds, stable=True)
    Ds, v, pi, A = Ds[perm], v[perm].contiguous(), pi[perm].contiguous(), A[perm][:, perm].contiguous()
    rank = torch.empty_like(perm)
    rank[perm] = torch.arange(K, device=dev)
    sp = sp.long()
    sp = torch.where(sp >= 0, rank[sp.clamp(min=0)], sp)
    state, _ = _hmm_viterbi_any(pos, off, kind, v, A, pi)
    G = torch.where(ok[:, None], g_sum, zero).sum(dim=0)[perm]
    n_inc = int(torch.where(ok, (toff[1:] - toff[:-1] - 1).to(dev), torch.zeros((), dtype=torch.int64, device=dev)).sum())
    return _hmm_out({"Ds": Ds, "M": A, "p0": pi, "loglik": trace[-1], "n_iter": len(trace), "converged": converged,
                     "loglik_trace": np.asarray(trace), "bic": -2.0 * trace[-1] + (K * K + K - 1) * float(np.log(max(n_inc, 1))),
                     "n_tracks_used": int(ok.sum()), "n_increments": n_inc, "gamma": gamma[:, perm], "state": state.long(),
                     "state_posterior": sp, "occupancy": G / G.sum()}, kind)


# ----------------------------------------------------------------------------------------------------------------------
# stage drift: the motion all tracks share, from their frame-to-frame increments (csrc/drift.hip)
# ----------------------------------------------------------------------------------------------------------------------
_DRIFT_THREADS = 256           # csrc/drift.hip: partial sums of a frame's mean
_DRIFT_SCAN_BLOCK = 256        # csrc/drift.hip: frames per block of the running sum
_DRIFT_MODES = {"mean": 0, "median": 1}
_SIGN64 = np.uint64(1 << 63)


def _drift_keys(d):
    """float64 -> uint64 keys whose unsigned order is the order of the values, -0 before +0 (csrc/drift.hip::drift_key)."""
    u = np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)
    return np.where(u >= _SIGN64, ~u, u | _SIGN64)


def _drift_unkeys(k):
    return np.where(k >= _SIGN64, k & ~_SIGN64, ~k).view(np.float64)


def _drift_frames_numpy(pos, pair_row, frame_offsets, mode):
    """The arithmetic of csrc/drift.hip::drift_frames_kernel in its order (include/mivit_hip.h, mivit_drift_frames).  Mean: 256
    partial sums, entry t over the increments t, t + 256, .. of the frame from +0 (np.cumsum over the rounds is sequential;
    the zeros that pad the last round add nothing to a sum that started at +0), folded in halves.  Median: np.sort of the
    keys that order -0 before +0.  pos [N, 2] float64, pair_row [M], frame_offsets [F + 1] integers -> stat [F, 2], bitwise
    the kernel's."""
    F, W = len(frame_offsets) - 1, _DRIFT_THREADS
    stat = np.zeros((F, 2))
    pair_row = np.asarray(pair_row, dtype=np.int64)
    with np.errstate(all="ignore"):
        d = pos[pair_row] - pos[pair_row - 1] if len(pair_row) else np.zeros((0, 2))
        for f in range(F):
            a, b = int(frame_offsets[f]), int(frame_offsets[f + 1])
            n = b - a
            if n <= 0:
                continue
            x = d[a:b]
            if mode == 0:
                rounds = -(-n // W)
                pad = np.zeros((rounds + 1, W, 2))                                          # round 0: the +0 the sums start from
                pad[1:].reshape(-1, 2)[:n] = x
                s = np.cumsum(pad, axis=0)[-1]
                half = W // 2
                while half > 0:
                    s[:half] = s[:half] + s[half:2 * half]
                    half //= 2
                stat[f] = s[0] / float(n)
            else:
                for axis in range(2):
                    col = x[:, axis]
                    if np.isnan(col).any():
                        stat[f, axis] = np.nan
                        continue
                    v = _drift_unkeys(np.sort(_drift_keys(col)))
                    stat[f, axis] = v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0
    return stat


def _drift_integrate_numpy(stat, n_pairs, half_window):
    """The arithmetic of csrc/drift.hip::drift_velocity_kernel and drift_scan_kernel in their order (mivit_drift_integrate):
    the window's numerator from +0 in ascending frame, each product rounded first; the running sum in blocks of 256 frames,
    np.cumsum inside a block and over the block totals.  stat [F, 2] float64, n_pairs [F] integers -> (velocity, drift)
    [F, 2], bitwise the kernels'."""
    F, B = len(stat), _DRIFT_SCAN_BLOCK
    vel = np.zeros((F, 2))
    with np.errstate(all="ignore"):
        if F > 1 and half_window == 0:
            vel[1:] = stat[1:]
        elif F > 1:
            h = min(int(half_window), F)
            c = np.maximum(np.asarray(n_pairs, dtype=np.int64), 0)
            w = c.astype(np.float64)[:, None] * stat
            num, den = np.zeros((F, 2)), np.zeros(F, np.int64)
            f = np.arange(F)
            for off in range(-h, h + 1):
                g = f + off
                ok = (g >= 1) & (g <= F - 1) & (f >= 1)
                g = np.clip(g, 0, F - 1)
                num = np.where(ok[:, None], num + w[g], num)
                den = den + np.where(ok, c[g], 0)
            vel = np.where((den > 0)[:, None], num / den.astype(np.float64)[:, None], 0.0)
        nb = -(-F // B)
        pad = np.zeros((nb * B, 2))
        pad[:F] = vel
        drift = np.cumsum(pad.reshape(nb, B, 2), axis=1)
        if nb > 1:
            drift[1:] = np.cumsum(drift[:-1, B - 1], axis=0)[:, None, :] + drift[1:]
    return vel, drift.reshape(nb * B, 2)[:F].copy()


def _drift_pairs(pos, fr, off, usable, F, min_pairs):
    """The increments estimate_drift uses, as the kernel takes them: pos [N, 2] float64, fr [N] and off [n_tracks + 1] int64,
    usable [N] bool or None, tensors on one device -> (pair_row [M] int64, the later row of every increment, grouped by its
    frame and in ascending row within a frame; n_pairs [F] int64, after min_pairs; frame_offsets [F + 1] int64; n_rejected).
    Torch ops on the device: no loop over frames or tracks."""
    n, dev = pos.shape[0], pos.device
    if n >= 2:
        first = torch.zeros(n, dtype=torch.bool, device=dev)
        first[off[:-1][off[1:] > off[:-1]]] = True
        cand = ~first[1:] & (fr[1:] - fr[:-1] == 1)
        if usable is not None:
            cand &= usable[1:] & usable[:-1]
        finite = torch.isfinite(pos).all(dim=1)
        finite = finite[1:] & finite[:-1]
        n_rejected = int((cand & ~finite).sum())
        rows = torch.nonzero(cand & finite, as_tuple=True)[0] + 1
    else:
        n_rejected, rows = 0, torch.zeros(0, dtype=torch.int64, device=dev)
    pf = fr[rows]
    order = torch.argsort(pf, stable=True)                      # rows stay in ascending order within a frame
    rows, pf = rows[order], pf[order]
    counts = torch.bincount(pf, minlength=F)
    enough = counts >= min_pairs
    rows = rows[enough[pf]]
    counts = torch.where(enough, counts, torch.zeros((), dtype=counts.dtype, device=dev))
    frame_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
    return rows, counts, frame_offsets, n_rejected


def _check_frames(frames, n, what="frames"):
    if len(frames.shape) != 1 or frames.shape[0] != n:
        raise ValueError(f"{what} must be [N] with one entry per row, got {tuple(frames.shape)} for {n} rows")
    kind = frames.dtype
    if torch.is_tensor(frames):
        integer = not (kind == torch.bool or kind.is_floating_point or kind.is_complex)
    else:
        integer = kind.kind in "iu"
    if not integer:
        raise ValueError(f"{what} must be integers, got {kind}")


def estimate_drift(positions, frames, offsets, n_frames=None, estimator="mean", smoothing=0, min_pairs=1, use=None):
    """The drift of the stage from the tracks themselves (trackpy's compute_drift): positions [N, 2] (y, x) and frames [N]
    (integers >= 0) sorted by track and by frame within a track, offsets [n_tracks + 1] (CSR), as tracking.
    tracks_table_by_track and simulate_movie's truth give them -> dict of the input's kind:
        drift    [F, 2] float64   the stage offset of every frame relative to frame 0: subtract_drift takes it
        velocity [F, 2] float64   its increment per frame, velocity[0] = 0
        n_pairs  [F] int32        the increments each frame's estimate rests on (0 where there were fewer than min_pairs)
        n_rejected                increments left out because a position was not finite
    F = n_frames (default max(frames) + 1).  An increment pos[r] - pos[r - 1] is used when rows r - 1 and r are consecutive
    rows of one track, their frames differ by exactly 1 (the increment across a gap is left out), both are usable (use [N]
    bool, default all: pass ~filled for a gap-closed table) and both positions are finite; it belongs to the later frame.  Per
    frame the estimator is the "mean" of its increments or their exact "median" per axis (robust against a few tracks that
    jump), 0 where a frame has fewer than min_pairs.  smoothing = h > 0 replaces each frame's value by the mean over the
    frames max(1, f - h) .. min(F - 1, f + h) weighted by n_pairs; h = 0 keeps it as it is.  drift is the running sum.
    include/mivit_hip.h has the arithmetic and every summation order.

    Subtracting the mean of n increments removes 1 / n of every particle's own motion with it: D of the corrected tracks
    comes out near (1 - 1 / n) D, and smoothing over 2 h + 1 frames reduces the loss to about 1 / ((2 h + 1) n).

    The pair list is a handful of torch ops on the input's device (a stable sort by frame, bincount, cumsum; no loop over
    frames or tracks).  CUDA tensors go to the kernels (csrc/drift.hip, no atomics: the same bits in every run; the median
    takes at most ops.DRIFT_MAX_PAIRS increments a frame), anything else to the numpy restatements, bitwise equal."""
    if estimator not in _DRIFT_MODES:
        raise ValueError(f"estimator must be 'mean' or 'median', got {estimator!r}")
    if isinstance(smoothing, bool) or int(smoothing) != smoothing or smoothing < 0:
        raise ValueError(f"smoothing must be an integer >= 0 (the half window in frames), got {smoothing}")
    if isinstance(min_pairs, bool) or int(min_pairs) != min_pairs or min_pairs < 1:
        raise ValueError(f"min_pairs must be an integer >= 1, got {min_pairs}")
    if len(positions.shape) != 2 or positions.shape[1] != 2:
        raise ValueError(f"positions must be [N, 2], got {tuple(positions.shape)}")
    is_t = torch.is_tensor(positions)
    given = [frames, offsets] + ([] if use is None else [use])
    if any(torch.is_tensor(g) != is_t for g in given):
        raise ValueError("positions, frames, offsets and use must all be tensors or all be arrays")
    if is_t and any(g.device != positions.device for g in given):
        raise ValueError(f"positions on {positions.device}, the other arguments elsewhere")
    if not is_t:
        positions, frames, offsets = np.asarray(positions, dtype=np.float64), np.asarray(frames), np.asarray(offsets)
        use = None if use is None else np.asarray(use)
    n = positions.shape[0]
    _check_frames(frames, n)
    _check_offsets(offsets, n)
    if use is not None and (tuple(use.shape) != (n,) or use.dtype != (torch.bool if is_t else np.bool_)):
        raise ValueError(f"use must be bool [N], got {use.dtype} {tuple(use.shape)}")
    if is_t:
        as_t = lambda a: a.detach()                                                               # noqa: E731
    else:
        as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else a.copy())     # noqa: E731
    pos, fr, off = as_t(positions).double().contiguous(), as_t(frames).long(), as_t(offsets).long()
    dev = pos.device
    f_lo, f_hi = (int(fr.min()), int(fr.max())) if n else (0, -1)
    if f_lo < 0:
        raise ValueError(f"frames must be >= 0, got {f_lo}")
    if n_frames is None:
        F = f_hi + 1
    else:
        if isinstance(n_frames, bool) or int(n_frames) != n_frames or n_frames < 0:
            raise ValueError(f"n_frames must be None or an integer >= 0, got {n_frames}")
        F = int(n_frames)
        if f_hi >= F:
            raise ValueError(f"frame {f_hi} in a movie of n_frames = {F}")
    usable = None if use is None else as_t(use)
    rows, counts, frame_offsets, n_rejected = _drift_pairs(pos, fr, off, usable, F, int(min_pairs))
    mode, h = _DRIFT_MODES[estimator], int(smoothing)
    if dev.type == "cuda":
        from .. import ops
        n_pairs = counts.int()
        stat = ops.drift_frames(pos, rows.int(), frame_offsets.int(), mode)
        velocity, drift = ops.drift_integrate(stat, n_pairs, h)
        return {"drift": drift, "velocity": velocity, "n_pairs": n_pairs, "n_rejected": n_rejected}
    stat = _drift_frames_numpy(pos.numpy(), rows.numpy(), frame_offsets.numpy(), mode)
    velocity, drift = _drift_integrate_numpy(stat, counts.numpy(), h)
    out = {"drift": drift, "velocity": velocity, "n_pairs": counts.numpy().astype(np.int32)}
    if is_t:
        out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}
    out["n_rejected"] = n_rejected
    return out


def subtract_drift(positions, frames, drift):
    """positions [N, 2] - drift[frames] (trackpy's subtract_drift): drift [F, 2] as estimate_drift returns it, frames [N]
    integers in [0, F); arrays or tensors on one device, the result of the input's kind."""
    if len(positions.shape) != 2 or positions.shape[1] != 2:
        raise ValueError(f"positions must be [N, 2], got {tuple(positions.shape)}")
    if len(drift.shape) != 2 or drift.shape[1] != 2:
        raise ValueError(f"drift must be [F, 2], got {tuple(drift.shape)}")
    is_t = torch.is_tensor(positions)
    if torch.is_tensor(frames) != is_t or torch.is_tensor(drift) != is_t:
        raise ValueError("positions, frames and drift must all be tensors or all be arrays")
    if not is_t:
        positions, frames, drift = np.asarray(positions), np.asarray(frames), np.asarray(drift)
    elif frames.device != positions.device or drift.device != positions.device:
        raise ValueError(f"positions on {positions.device}, frames on {frames.device}, drift on {drift.device}")
    _check_frames(frames, positions.shape[0])
    if positions.shape[0] and (int(frames.min()) < 0 or int(frames.max()) >= drift.shape[0]):
        raise ValueError(f"frames must lie in [0, {drift.shape[0]}), got {int(frames.min())} .. {int(frames.max())}")
    return positions - drift[frames.long() if is_t else frames.astype(np.int64)]


# ----------------------------------------------------------------------------------------------------------------------
# maximum-likelihood D per track from rows of known variance, with a standard error (csrc/likelihood.hip)
# ----------------------------------------------------------------------------------------------------------------------
_ML_CANDIDATES, _ML_ROUNDS, _ML_U_LO, _ML_U_HI = 64, 6, -20.0, 4.0
# what the three fits of this family share (csrc/track_ml.h has the same pieces for the kernels)
_ML_LN2 = 0.6931471805599453                      # np.log(2)
_ML_H = 1.0 / 64.0                                # the step of the curvature's differences
_ML_EXP_H, _ML_EXP_MH = 1.0157477085866857, 0.9844964370054085           # np.exp(1 / 64), np.exp(-1 / 64)


def _ml_usable(pos, var, frames, use, offsets):
    """The usable rows of every range, a list of n index arrays into the rows: a row is usable when its flag is set (use
    None: all are), both coordinates are finite and both variances are finite and >= 0 (var None: zeros).  frames plays no
    part; it is taken so that the restatements hand over their arguments as they got them."""
    ok = np.isfinite(pos).all(axis=1)
    if var is not None:
        with np.errstate(invalid="ignore"):
            ok &= ((var >= 0.0) & (var < np.inf)).all(axis=1)
    if use is not None:
        ok &= use.astype(bool)
    return [int(offsets[k]) + np.nonzero(ok[int(offsets[k]):int(offsets[k + 1])])[0] for k in range(len(offsets) - 1)]


def _ml_padded(rows, sel, pos, var, frames, offsets):
    """The usable rows (rows: of _ml_usable) of the ranges sel, in the order given, padded with zeros to the longest: -> (X
    [ns, Mx, 2], V [ns, Mx, 2], Fr [ns, Mx] int64); a row's frame is its place in its range where frames is None"""
    Mx = max([len(rows[k]) for k in sel], default=0)
    X, V, Fr = np.zeros((len(sel), Mx, 2)), np.zeros((len(sel), Mx, 2)), np.zeros((len(sel), Mx), np.int64)
    for i, k in enumerate(sel):
        r = rows[k]
        X[i, :len(r)] = pos[r]
        if var is not None:
            V[i, :len(r)] = var[r]
        Fr[i, :len(r)] = frames[r] if frames is not None else r - int(offsets[k])
    return X, V, Fr


def _ml_prod_mul(pm, pe, x):
    """one factor more into the determinant of the first len(x) ranges, kept as a product rescaled exactly: pm the mantissa in
    [0.5, 1), pe the integer exponent, both changed in place"""
    m, ex = np.frexp(pm[:len(x)] * x)
    pm[:len(x)] = m
    pe[:len(x)] += ex


def _ml_finish_cost(pm, pe, Q, inc, bad):
    """-2 log L [n, C] = log det (the product pm 2^pe) + Q + 2 inc log 2 pi; +inf where bad and where it is not below +inf"""
    cost = ((np.log(pm) + pe.astype(np.float64) * _ML_LN2) + Q) + (2 * inc).astype(np.float64)[:, None] * _LOG_2PI
    return np.where(bad | ~(cost < np.inf), np.inf, cost)


def _ml_d_ref(d, g, inc, dt):
    """The reference scale sum d^2 (both axes) / (4 dt sum g) over the first inc [n] increments of each range: d [n, M, 2] the
    increments, g [n, M] their gaps in frames; the sum of the squares in the kernels' order"""
    live = np.arange(d.shape[1])[None, :] < inc[:, None]
    S = np.cumsum(np.where(live, d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1], 0.0), axis=1)[:, -1]
    G = np.where(live, g, 0).sum(axis=1)
    return S / ((4.0 * dt) * G.astype(np.float64))


def _ml_curvature(cp, c0, cm):
    """half the second difference of the cost over h^2, h = 1 / 64"""
    return ((cp - c0) + (cm - c0)) * 2048.0


def _ml_hessian(c):
    """The 2 x 2 observed information in (u, v) from the nine costs c [..., 9] of the stencil, c[..., 3 a + b] at (u + (a - 1)
    h, v + (b - 1) h) -> (uu, vv, uv, det, whether it is positive definite)"""
    c0 = c[..., 4]
    uu = _ml_curvature(c[..., 7], c0, c[..., 1])
    vv = _ml_curvature(c[..., 5], c0, c[..., 3])
    uv = ((c[..., 8] - c[..., 6]) - (c[..., 2] - c[..., 0])) * 512.0       # 1 / (8 h^2)
    det = uu * vv - uv * uv
    return uu, vv, uv, det, (uu > 0.0) & (vv > 0.0) & (det > 0.0) & (det < np.inf)


def _ml_cost(Dc, d, g, V, inc, dt, R):
    """-2 log L of csrc/likelihood.hip::ml_cost for the candidates Dc [n, C] of n ranges at once: d [n, >= inc[0], 2] the
    increments, g [n, >= inc[0]] their gaps in frames, V [n, >= inc[0] + 1, 2] the row variances, inc [n] >= 1 the increments
    of each range IN DESCENDING ORDER (the ranges still running at step k are a prefix).  Elementwise the kernel's operations
    in its order; the two differ in log alone."""
    n, C = Dc.shape
    c1 = (2.0 * Dc) * dt
    cR, tR = R * c1, 2.0 * R
    Q, pm, pe = np.zeros((n, C)), np.full((n, C), 0.5), np.ones((n, C), np.int64)
    bad = np.zeros((n, C), bool)
    rinv, z = np.zeros((2, n, C)), np.zeros((2, n, C))
    with np.errstate(all="ignore"):
        for k in range(int(inc[0]) if n else 0):
            na = int(np.count_nonzero(inc > k))
            base = c1[:na] * (g[:na, k].astype(np.float64) - tR)[:, None]
            for ax in (0, 1):
                pv, v, dd = V[:na, k, ax][:, None], V[:na, k + 1, ax][:, None], d[:na, k, ax][:, None]
                a = (base + pv) + v
                if k == 0:
                    e, zz = a, np.broadcast_to(dd, a.shape)
                else:
                    b = cR[:na] - pv
                    l = b * rinv[ax, :na]
                    e = a - l * b
                    zz = dd - l * z[ax, :na]
                bad[:na] |= ~(e > 0.0)
                r = 1.0 / e
                Q[:na] = Q[:na] + (zz * zz) * r
                _ml_prod_mul(pm, pe, e)
                rinv[ax, :na], z[ax, :na] = r, zz
        return _ml_finish_cost(pm, pe, Q, inc, bad)


def _diffusion_ml_numpy(pos, var, frames, use, offsets, dt, R):
    """The arithmetic of csrc/likelihood.hip::ml_kernel in its order (include/mivit_hip.h, mivit_track_diffusion_ml), all
    ranges at once: pos [N, 2] float64, var [N, 2] float64 or None, frames [N] integers or None, use [N] bool or None, offsets
    [n + 1] int64 -> (D, D_std, loglik [n] float64, n_increments, status [n] int32).  The same recurrence, the same
    determinant as a product rescaled by frexp, the same search; np.argmin returns the lowest index among equal minima.
    Differs from the kernel in log and exp2 alone."""
    n = len(offsets) - 1
    D, D_std, loglik = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    status = np.ones(n, np.int32)
    rows = _ml_usable(pos, var, frames, use, offsets)
    n_inc = np.array([max(len(r) - 1, 0) for r in rows], np.int32).reshape(n)
    sel = np.nonzero(n_inc >= 2)[0]
    if not len(sel):
        return D, D_std, loglik, n_inc, status
    sel = sel[np.argsort(-n_inc[sel], kind="stable")]                      # descending: the ranges still running are a prefix
    inc = n_inc[sel].astype(np.int64)
    ns = len(sel)
    X, V, Fr = _ml_padded(rows, sel, pos, var, frames, offsets)
    d, g = X[:, 1:] - X[:, :-1], Fr[:, 1:] - Fr[:, :-1]
    with np.errstate(all="ignore"):
        D_ref = _ml_d_ref(d, g, inc, dt)
        lo, hi = np.full(ns, _ML_U_LO), np.full(ns, _ML_U_HI)
        all_lo, all_hi = np.ones(ns, bool), np.ones(ns, bool)
        lane, each = np.arange(_ML_CANDIDATES, dtype=np.float64), np.arange(ns)
        Db = np.zeros(ns)
        for _ in range(_ML_ROUNDS):
            step = (hi - lo) / 63.0
            Dj = D_ref[:, None] * np.exp2(lo[:, None] + lane[None, :] * step[:, None])
            j = np.argmin(_ml_cost(Dj, d, g, V, inc, dt, R), axis=1)
            all_lo &= j == 0
            all_hi &= j == _ML_CANDIDATES - 1
            Db = Dj[each, j]
            jl, jh = np.maximum(j - 1, 0), np.minimum(j + 1, _ML_CANDIDATES - 1)
            lo, hi = lo + jl.astype(np.float64) * step, lo + jh.astype(np.float64) * step
        st = np.where(all_lo, 2, np.where(all_hi, 3, 0)).astype(np.int32)
        Db = np.where(all_lo, 0.0, Db)
        c = _ml_cost(np.stack([Db, Db * _ML_EXP_H, Db * _ML_EXP_MH], axis=1), d, g, V, inc, dt, R)
        info = _ml_curvature(c[:, 1], c[:, 0], c[:, 2])
        curved = (info > 0.0) & (info < np.inf)
        D[sel], loglik[sel] = Db, -0.5 * c[:, 0]
        D_std[sel] = np.where(curved & (st != 2), Db / np.sqrt(info), np.nan)
        status[sel] = np.where(~curved & (st == 0), 4, st)
    return D, D_std, loglik, n_inc, status


def _ml_arguments(positions, offsets, variances, frames, use, dt):
    """The argument handling that estimate_diffusion_ml and estimate_anomalous_ml share: the checks, then everything as torch
    tensors on the input's device -> (is_t, pos [N, 2] float64, off [n + 1] int64, var [N, 2] float64 or None, fr [N] int64 or
    None, usable [N] bool or None)."""
    if not 0.0 < float(dt) < float("inf"):
        raise ValueError(f"dt must be positive and finite, got {dt}")
    if len(positions.shape) != 2 or positions.shape[1] != 2:
        raise ValueError(f"positions must be [N, 2], got {tuple(positions.shape)}")
    is_t = torch.is_tensor(positions)
    scalar_var = variances is not None and not torch.is_tensor(variances) and np.ndim(variances) == 0
    given = [offsets] + [g for g in (None if scalar_var else variances, frames, use) if g is not None]
    if any(torch.is_tensor(g) != is_t for g in given):
        raise ValueError("positions, offsets, variances, frames and use must all be tensors or all be arrays")
    if is_t and any(g.device != positions.device for g in given):
        raise ValueError(f"positions on {positions.device}, the other arguments elsewhere")
    if not is_t:
        positions, offsets = np.asarray(positions, dtype=np.float64), np.asarray(offsets)
        variances = variances if variances is None or scalar_var else np.asarray(variances, dtype=np.float64)
        frames = None if frames is None else np.asarray(frames)
        use = None if use is None else np.asarray(use)
    n = positions.shape[0]
    _check_offsets(offsets, n)
    if scalar_var:
        if not 0.0 <= float(variances) < float("inf"):
            raise ValueError(f"a variance must be >= 0 and finite, got {variances}")
    elif variances is not None and tuple(variances.shape) not in ((n,), (n, 2)):
        raise ValueError(f"variances must be [N, 2], [N] or a number, got {tuple(variances.shape)} for {n} rows")
    if frames is not None:
        _check_frames(frames, n)
    if use is not None and (tuple(use.shape) != (n,) or use.dtype != (torch.bool if is_t else np.bool_)):
        raise ValueError(f"use must be bool [N], got {use.dtype} {tuple(use.shape)}")
    if is_t:
        as_t = lambda a: a.detach()                                                               # noqa: E731
    else:
        as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else a.copy())     # noqa: E731
    pos, off = as_t(positions).double().contiguous(), as_t(offsets).long()
    if variances is None or (scalar_var and float(variances) == 0.0):
        var = None
    elif scalar_var:
        var = torch.full((n, 2), float(variances), dtype=torch.float64, device=pos.device)
    else:
        var = as_t(variances).double()
        var = (var[:, None].expand(n, 2) if var.dim() == 1 else var).contiguous()
    fr = None if frames is None else as_t(frames).long()
    if fr is not None and n > 1:
        inside = torch.ones(n - 1, dtype=torch.bool, device=pos.device)    # row r and row r + 1 belong to one range
        starts = off[1:-1]
        inside[starts[(starts > 0) & (starts < n)] - 1] = False
        if bool(((fr[1:] <= fr[:-1]) & inside).any()):
            raise ValueError("frames must rise within every range")
        if int(fr.min()) < -2 ** 31 or int(fr.max()) >= 2 ** 31:
            raise ValueError("frames must fit 32 bits")
    usable = None if use is None else as_t(use).contiguous()
    return is_t, pos, off, var, fr, usable


def _ml_per_range(v, n, what, device, width=None):
    """a parameter given as a number (width: as [width]) or per range -> float64 tensor [n] ([n, width]) on the device"""
    v = v.detach().to(device, torch.float64) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, np.float64), device=device)
    shape = (n,) if width is None else (n, width)
    if v.dim() == (0 if width is None else 1) and (width is None or tuple(v.shape) == (width,)):
        v = v.expand(*shape)
    if tuple(v.shape) != shape:
        raise ValueError(f"{what} must be {'a number' if width is None else f'[{width}]'} or {list(shape)}, got {tuple(v.shape)}")
    return v.contiguous()


def _ml_dispatch(args, kernel, restated, keys):
    """The tail that the front ends of this family share.  args: what _ml_arguments returned.  CUDA tensors go to
    kernel(ops, pos, offsets int32, var, frames int32, use), everything else to restated(pos, var, frames, use, offsets) as
    numpy arrays (None stays None) -> dict of the outputs under keys, of the input's kind, n_increments and status as int64."""
    is_t, pos, off, var, fr, usable = args
    on_gpu = pos.device.type == "cuda"
    if on_gpu:
        from .. import ops
        got = kernel(ops, pos, off.int().contiguous(), var, None if fr is None else fr.int().contiguous(), usable)
    else:
        got = restated(*(None if t is None else t.numpy() for t in (pos, var, fr, usable, off)))
    out = dict(zip(keys, got if isinstance(got, tuple) else (got,)))
    for k in ("n_increments", "status"):
        if k in out:
            out[k] = out[k].long() if on_gpu else out[k].astype(np.int64)
    return {k: torch.from_numpy(v) for k, v in out.items()} if is_t and not on_gpu else out


def estimate_diffusion_ml(positions, offsets, variances=None, frames=None, use=None, dt=1.0, blur=0.0):
    """The maximum-likelihood diffusion coefficient of every track with its standard error, from rows that each carry their
    own localisation variance (Berglund 2010; Michalet & Berglund 2012; Relich et al. 2016): positions [N, 2] (y, x) sorted
    by track and by frame, offsets [n + 1] (CSR, from 0 to N: tracks, or the seg_offsets / run_offsets of segment_tracks and
    estimate_track_diffusion) -> dict of the input's kind:
        D_ml         [n] float64   in pixels^2 per unit of dt; 0 for a track that does not move within its noise (status 2)
        D_ml_std     [n] float64   its standard error, D_ml / sqrt(observed information in ln D)
        loglik       [n] float64   the log-likelihood at D_ml
        n_increments [n] int64     the increments between usable rows
        status       [n] int64     0 fine; 1 fewer than 2 increments (NaN); 2 the minimum at the lower end of the search
                                   (D_ml = 0, D_ml_std NaN); 3 at its upper end; 4 the curvature is not positive (D_ml_std NaN)
    variances: the variance of each coordinate, [N, 2], or [N] (both axes alike), or one number, or None for 0: the squared
    Cramer-Rao bounds (y_std^2, x_std^2) of fit_spots_mle are what it was made for.  frames [N] integers rising within a
    track (None: consecutive rows are consecutive frames); a track may have gaps, and a gap-closed table need not be filled.
    use [N] bool (None: all): a row is left out where it is False, where a coordinate is not finite, and where a variance is
    negative or not finite; the increment then bridges its neighbours like any other gap.  blur is the motion-blur
    coefficient R in [0, 1/4] (0: instantaneous exposure, 1/6: exposure over the whole frame).

    The increments of a track are zero-mean Gaussian with a tridiagonal covariance (2 D dt (g - 2 R) + v_k + v_{k+1} on the
    diagonal, 2 R D dt - v_{k+1} beside it), the two axes independent and sharing D.  The likelihood is evaluated by the
    LDL^T recurrence and maximised by a fixed grid search over log2 D: six rounds of 64 candidates, from D_ref 2^-20 to D_ref
    2^4 with D_ref = <d^2> / (4 dt <g>); include/mivit_hip.h has every operation.  Unlike D_cve it uses rows of different
    quality for what they are worth and needs no gap-free table; unlike D_msd and segments["D_mle"] it is not biased by
    localisation noise and motion blur.  CUDA tensors go to the kernel (csrc/likelihood.hip: one wave per track, no limit on
    its length), numpy arrays and CPU tensors to the numpy restatement, which differs from it in log and exp2 alone."""
    if not 0.0 < float(dt) < float("inf"):
        raise ValueError(f"dt must be positive and finite, got {dt}")
    if not 0.0 <= float(blur) <= 0.25:
        raise ValueError(f"blur must lie in [0, 1/4], got {blur}")
    return _ml_dispatch(_ml_arguments(positions, offsets, variances, frames, use, dt),
                        lambda ops, pos, off, var, fr, usable: ops.track_diffusion_ml(pos, off, var, fr, usable, float(dt), float(blur)),
                        lambda *rows: _diffusion_ml_numpy(*rows, float(dt), float(blur)),
                        ("D_ml", "D_ml_std", "loglik", "n_increments", "status"))


# ----------------------------------------------------------------------------------------------------------------------
# maximum-likelihood anomalous exponent per track from rows of known variance, with error bars (csrc/fbm_ml.hip)
# ----------------------------------------------------------------------------------------------------------------------
FBM_ML_MAX_ROWS, FBM_ML_MAX_SPAN = 129, 1199      # csrc/fbm_ml.hip: usable rows of a range, largest - smallest usable frame
_FBM_GRID, _FBM_ROUNDS, _FBM_U_LO, _FBM_U_HI, _FBM_TERMS = 8, 20, -12.0, 4.0, 30


def fbm_structure(alpha, lag, exposure=0.0):
    """The structure function S of fractional Brownian motion averaged over an exposure E in [0, 1] of a frame, at integer
    lags (in frames; the sign does not matter), alpha and lag broadcast against each other: the per-axis variance of the
    difference of two averaged positions that lie `lag` frames apart is 2 D dt (S(lag) - S(0)).  E = 0: |lag|^alpha.  E > 0: the double integral of |lag + s - t|^alpha over the exposure,
    2 E^alpha / ((alpha + 1)(alpha + 2)) at lag 0, the closed form where E > |lag| / 2 and a series of 30 terms in (E / lag)^2
    elsewhere, which does not cancel.  The operations of csrc/fbm_ml.hip::fm_structure in their order."""
    alpha, tau = np.broadcast_arrays(np.asarray(alpha, np.float64), np.abs(np.asarray(lag)).astype(np.float64))
    E = float(exposure)
    with np.errstate(all="ignore"):
        if E == 0.0:
            return np.where(tau == 0, 0.0, np.power(tau, alpha))
        a12 = (alpha + 1.0) * (alpha + 2.0)
        p = alpha + 2.0
        closed = ((np.power(tau + E, p) + np.power(np.abs(tau - E), p)) - 2.0 * np.power(tau, p)) / ((E * E) * a12)
        x = E / np.where(tau == 0, 1.0, tau)
        x2 = x * x
        term, total = np.ones(tau.shape), np.ones(tau.shape)
        for m in range(1, _FBM_TERMS + 1):
            tm = float(2 * m)
            term = (term * (((alpha - tm + 2.0) * (alpha - tm + 1.0)) / ((tm + 1.0) * (tm + 2.0)))) * x2
            total = total + term
        return np.where(tau == 0, (2.0 * np.power(E, alpha)) / a12, np.where(E > 0.5 * tau, closed, np.power(tau, alpha) * total))


def _fbm_usable_rows(pos, var, frames, use, offsets):
    """-> per range (X [M, 2], V [M, 2], F [M] int64) of its usable rows"""
    rows = _ml_usable(pos, var, frames, use, offsets)
    return [tuple(t[0] for t in _ml_padded(rows, [k], pos, var, frames, offsets)) for k in range(len(rows))]


def _fbm_over_limit(F):
    return len(F) > FBM_ML_MAX_ROWS or (len(F) > 0 and int(F.max()) - int(F.min()) > FBM_ML_MAX_SPAN)


def _fbm_cost(alpha, D, X, V, F, dt, E):
    """-2 log L of one range (X [m + 1, 2], V [m + 1, 2], F [m + 1], m >= 1) at the candidates alpha [C], D [C]: the dense
    covariance of include/mivit_hip.h (mivit_track_fbm_loglik) per axis, LAPACK's Cholesky, +inf where it is not positive
    definite or the cost is not below +inf."""
    m = len(X) - 1
    d = X[1:] - X[:-1]
    lo, hi = F[:-1] - F.min(), F[1:] - F.min()
    with np.errstate(all="ignore"):
        tab = fbm_structure(alpha[:, None], np.arange(int(F.max() - F.min()) + 1)[None, :], E)
        q = ((tab[:, np.abs(hi[:, None] - lo[None, :])] + tab[:, np.abs(lo[:, None] - hi[None, :])])
             - tab[:, np.abs(hi[:, None] - hi[None, :])]) - tab[:, np.abs(lo[:, None] - lo[None, :])]
        base = (D * dt)[:, None, None] * q
        cost = np.full(len(alpha), float(2 * m) * _LOG_2PI)
        for ax in (0, 1):
            v = V[:, ax]
            C = base + (np.diag(v[:-1] + v[1:]) - np.diag(v[1:-1], 1) - np.diag(v[1:-1], -1))[None]
            L = np.full(C.shape, np.nan)
            try:
                L = np.linalg.cholesky(C)
            except np.linalg.LinAlgError:
                for c in range(len(C)):
                    try:
                        L[c] = np.linalg.cholesky(C[c])
                    except np.linalg.LinAlgError:
                        pass
            fine = np.isfinite(L).all(axis=(1, 2))
            L[~fine] = np.eye(m)
            z = np.linalg.solve(L, np.broadcast_to(d[:, ax, None], (len(C), m, 1)))[..., 0]
            cost = cost + np.where(fine, 2.0 * np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1) + (z * z).sum(axis=1), np.inf)
        return np.where(cost < np.inf, cost, np.inf)


def _fbm_loglik_numpy(pos, var, frames, use, offsets, dt, E, alpha, D):
    """csrc/fbm_ml.hip's mivit_track_fbm_loglik restated -> (loglik [n] float64, n_increments, status [n] int32)"""
    n = len(offsets) - 1
    loglik, n_inc, status = np.full(n, np.nan), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k, (X, V, F) in enumerate(_fbm_usable_rows(pos, var, frames, use, offsets)):
        n_inc[k] = max(len(X) - 1, 0)
        if _fbm_over_limit(F):
            status[k] = 5
        elif n_inc[k] < 1:
            status[k] = 1
        elif not (0.0 < alpha[k] < 2.0 and 0.0 <= D[k] < np.inf):
            status[k] = 6
        else:
            loglik[k] = -0.5 * _fbm_cost(alpha[k:k + 1], D[k:k + 1], X, V, F, dt, E)[0]
    return loglik, n_inc, status


def _fbm_ml_numpy(pos, var, frames, use, offsets, dt, E):
    """The search of csrc/fbm_ml.hip (include/mivit_hip.h, mivit_track_fbm_ml) restated range by range: the same brackets,
    candidates, arg-min (np.argmin returns the lowest index among equal minima), stencil and statuses, on the cost of
    _fbm_cost -> (alpha, alpha_std, D, D_std, corr, loglik [n] float64, n_increments, status [n] int32).  Differs from the
    kernel in the order of the sums of the factorisation, in pow, exp2 and log."""
    from .generation import ALPHA_MAX, ALPHA_MIN
    n = len(offsets) - 1
    alpha, alpha_std, D, D_std, corr, loglik = (np.full(n, np.nan) for _ in range(6))
    n_inc, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    grid = np.arange(_FBM_GRID, dtype=np.float64)
    for k, (X, V, F) in enumerate(_fbm_usable_rows(pos, var, frames, use, offsets)):
        n_inc[k] = max(len(X) - 1, 0)
        if _fbm_over_limit(F):
            status[k] = 5
            continue
        if n_inc[k] < 3:
            status[k] = 1
            continue
        d = X[1:] - X[:-1]
        with np.errstate(all="ignore"):
            D_ref = np.cumsum(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])[-1] / ((4.0 * dt) * float(int(F[-1]) - int(F[0])))
            alo, ahi, ulo, uhi = ALPHA_MIN, ALPHA_MAX, _FBM_U_LO, _FBM_U_HI
            all_lo = all_hi = True
            for _ in range(_FBM_ROUNDS):
                sa, su = (ahi - alo) / 7.0, (uhi - ulo) / 7.0
                a_c = np.repeat(alo + grid * sa, _FBM_GRID)
                D_c = np.tile(D_ref * np.exp2(ulo + grid * su), _FBM_GRID)
                best = int(np.argmin(_fbm_cost(a_c, D_c, X, V, F, dt, E)))
                i, j = best >> 3, best & 7
                ab, ub = alo + float(i) * sa, ulo + float(j) * su
                alo, ahi, ulo, uhi = max(ab - 2.0 * sa, ALPHA_MIN), min(ab + 2.0 * sa, ALPHA_MAX), ub - 2.0 * su, ub + 2.0 * su
                all_lo, all_hi = all_lo and j == 0, all_hi and j == _FBM_GRID - 1
            Db = 0.0 if all_lo else float(D_ref * np.exp2(ub))
            a_s = np.repeat(ab + np.array([-1.0, 0.0, 1.0]) * _ML_H, 3)
            D_s = np.tile(np.array([Db * _ML_EXP_MH, Db, Db * _ML_EXP_H]), 3)
            c = _fbm_cost(a_s, D_s, X, V, F, dt, E)
            st = 2 if all_lo else (3 if all_hi else 0)
            loglik[k], D[k] = -0.5 * c[4], Db
            if st != 2:
                alpha[k] = ab
                Haa, Hdd, Had, det, pd = _ml_hessian(c)                    # u = alpha, v = ln D
                if ab - _ML_H >= ALPHA_MIN and ab + _ML_H <= ALPHA_MAX and pd:
                    alpha_std[k], D_std[k], corr[k] = np.sqrt(Hdd / det), Db * np.sqrt(Haa / det), -Had / np.sqrt(Haa * Hdd)
                elif st == 0:
                    st = 4
            status[k] = st
    return alpha, alpha_std, D, D_std, corr, loglik, n_inc, status


def _fbm_checked(exposure, dt):
    if not 0.0 < float(dt) < float("inf"):
        raise ValueError(f"dt must be positive and finite, got {dt}")
    if not 0.0 <= float(exposure) <= 1.0:
        raise ValueError(f"exposure must lie in [0, 1], got {exposure}")


def fbm_loglik(positions, offsets, alpha, D, variances=None, frames=None, use=None, dt=1.0, exposure=0.0):
    """The exact log-likelihood of every range under fractional Brownian motion with the exponent alpha and the generalised
    diffusion coefficient D (numbers, or one per range [n]; per-axis ensemble MSD 2 D dt lag^alpha), seen through an exposure
    over the first `exposure` of each frame and localisation noise of the rows' variances: the model of
    estimate_anomalous_ml at given parameters, to compare hypotheses with -> dict of the input's kind: loglik [n] float64
    (-inf where the covariance is not positive definite), n_increments [n] int64, status [n] int64 (0 fine, 1 no increment,
    5 over ops.FBM_ML_MAX_ROWS usable rows or ops.FBM_ML_MAX_SPAN frames, 6 alpha outside (0, 2) or D negative or not finite;
    loglik is NaN for 1, 5, 6).  The other arguments are those of estimate_diffusion_ml.  CUDA tensors go to the kernel
    (csrc/fbm_ml.hip), arrays and CPU tensors to the numpy restatement."""
    _fbm_checked(exposure, dt)
    args = _ml_arguments(positions, offsets, variances, frames, use, dt)
    n, device = args[2].numel() - 1, args[1].device
    a, Dv = _ml_per_range(alpha, n, "alpha", device), _ml_per_range(D, n, "D", device)
    return _ml_dispatch(args,
                        lambda ops, pos, off, var, fr, usable: ops.track_fbm_loglik(pos, off, a, Dv, var, fr, usable, float(dt), float(exposure)),
                        lambda *rows: _fbm_loglik_numpy(*rows, float(dt), float(exposure), a.numpy(), Dv.numpy()),
                        ("loglik", "n_increments", "status"))


def estimate_anomalous_ml(positions, offsets, variances=None, frames=None, use=None, dt=1.0, exposure=0.0):
    """The maximum-likelihood anomalous exponent and generalised diffusion coefficient of every track with their standard
    errors, from rows that each carry their own localisation variance: positions, offsets, variances, frames, use and dt as
    estimate_diffusion_ml takes them; exposure in [0, 1] is the part of a frame, from its start, over which the camera
    integrates (0: instantaneous, 1: the whole frame; at alpha = 1 it is blur = exposure / 6) -> dict of the input's kind:
        alpha_ml     [n] float64   the exponent, in [ALPHA_MIN, ALPHA_MAX] of helpers/generation; NaN for status 1, 2, 5
        alpha_ml_std [n] float64   its standard error
        D_alpha      [n] float64   the generalised coefficient: the per-axis ensemble MSD at a lag of k frames is
                                   2 D_alpha dt k^alpha, as fbm_single_state draws it; 0 for status 2
        D_alpha_std  [n] float64   its standard error
        corr         [n] float64   the correlation of the two estimates (of alpha and ln D)
        loglik       [n] float64   the log-likelihood at the estimates
        lr_brownian  [n] float64   2 (loglik - the loglik of estimate_diffusion_ml(..., blur=exposure / 6)): the likelihood
                                   ratio against Brownian motion, one more parameter
        n_increments [n] int64     the increments between usable rows
        status       [n] int64     0 fine; 1 fewer than 3 increments (NaN); 2 the track does not move within its noise
                                   (D_alpha = 0, alpha_ml and the bars NaN); 3 D at the upper end of every round; 4 the
                                   curvature is not positive definite or alpha_ml is within 1/64 of the end of its range
                                   (the estimates stay, the bars are NaN); 5 more than ops.FBM_ML_MAX_ROWS = 129 usable
                                   rows or usable frames that span more than ops.FBM_ML_MAX_SPAN = 1199 (NaN)
    Unlike estimate_alpha, the slope of log MSD against log lag, it is not biased by localisation noise and motion blur, uses
    gap-closed tracks without filling them and has an error bar.  The increments of a track are zero-mean Gaussian with a
    DENSE covariance (include/mivit_hip.h has every operation), factorised by Cholesky per candidate; the search is fixed, 20
    rounds of an 8 x 8 grid over alpha and log2 D that shrinks to the best candidate +- 2 cells, and the error bars come from
    the second differences of the log-likelihood with a step of 1/64 in alpha and in ln D.  CUDA tensors go to the kernel
    (csrc/fbm_ml.hip: one workgroup per track and candidate), arrays and CPU tensors to the numpy restatement with LAPACK's
    Cholesky, which differs from it in the order of sums, pow, exp2 and log."""
    _fbm_checked(exposure, dt)
    args = _ml_arguments(positions, offsets, variances, frames, use, dt)
    brownian = estimate_diffusion_ml(positions, offsets, variances, frames, use, dt, blur=float(exposure) / 6.0)["loglik"]
    out = _ml_dispatch(args,
                       lambda ops, pos, off, var, fr, usable: ops.track_fbm_ml(pos, off, var, fr, usable, float(dt), float(exposure)),
                       lambda *rows: _fbm_ml_numpy(*rows, float(dt), float(exposure)),
                       ("alpha_ml", "alpha_ml_std", "D_alpha", "D_alpha_std", "corr", "loglik", "n_increments", "status"))
    out["lr_brownian"] = 2.0 * (out["loglik"] - brownian)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# maximum-likelihood confinement radius per track from rows of known variance, with error bars (csrc/confined_ml.hip)
# ----------------------------------------------------------------------------------------------------------------------
_CF_GRID, _CF_ROUNDS, _CF_MIN_INCREMENTS = 8, 20, 4
_CF_U_LO, _CF_U_HI, _CF_W_LO, _CF_W_HI = -12.0, 4.0, -6.0, 18.0          # the first brackets of log2(D / D_ref), log2(s2 / S_ref)
_CF_FAST = 4.0                                                           # status 3 where lambda dt is above it


def _confined_cost(Dc, Sc, X, V, g, inc, dt, centre=None):
    """-2 log L of csrc/confined_ml.hip::cf_cost for the candidates (Dc, Sc) [n, C] (D and the stationary variance s2) of n
    ranges at once: X [n, >= inc[0] + 1, 2] the usable rows, V their variances, g [n, >= inc[0]] the gaps in frames, inc [n]
    >= 1 the increments of each range IN DESCENDING ORDER; centre [n, C, 2] given, or None to profile it -> (cost [n, C],
    centre [n, C, 2], Shh [n, C, 2]).  Elementwise the kernel's operations in its order (include/mivit_hip.h,
    mivit_track_confined_ml); the two differ in expm1 and log alone."""
    n, C = Dc.shape
    with np.errstate(all="ignore"):
        ldt = (Dc / Sc) * dt
        a = np.stack([np.broadcast_to(X[:, 0, ax][:, None], (n, C)) for ax in (0, 1)]).copy()
        b = np.zeros((2, n, C))
        P = np.stack([np.broadcast_to(V[:, 0, ax][:, None], (n, C)) for ax in (0, 1)]).copy()
        Syy, Syh, Shh = np.zeros((2, n, C)), np.zeros((2, n, C)), np.zeros((2, n, C))
        pm, pe = np.full((n, C), 0.5), np.ones((n, C), np.int64)
        bad = np.zeros((n, C), bool)
        for k in range(int(inc[0]) if n else 0):
            na = int(np.count_nonzero(inc > k))
            t = ldt[:na] * g[:na, k].astype(np.float64)[:, None]
            om = -np.expm1(-t)
            phi = 1.0 - om
            q = Sc[:na] * (-np.expm1(-(2.0 * t)))
            for ax in (0, 1):
                Pm = (phi * phi) * P[ax, :na] + q
                F = Pm + V[:na, k + 1, ax][:, None]
                bad[:na] |= ~(F > 0.0)
                r = 1.0 / F
                am = phi * a[ax, :na]
                eh = phi * b[ax, :na] + om
                ey = X[:na, k + 1, ax][:, None] - am
                K = Pm * r
                a[ax, :na] = am + K * ey
                b[ax, :na] = eh - K * eh
                P[ax, :na] = (1.0 - K) * Pm
                Syy[ax, :na] = Syy[ax, :na] + (ey * ey) * r
                Syh[ax, :na] = Syh[ax, :na] + (ey * eh) * r
                Shh[ax, :na] = Shh[ax, :na] + (eh * eh) * r
                _ml_prod_mul(pm, pe, F)
        if centre is None:
            pos_h = Shh > 0.0
            c = np.where(pos_h, Syh / Shh, np.nan)
            Q = np.where(pos_h, Syy - (Syh * Syh) / Shh, Syy)
        else:
            c = np.moveaxis(centre, 2, 0)
            Q = (Syy - ((2.0 * c) * Syh)) + (c * c) * Shh
        cost = _ml_finish_cost(pm, pe, Q[0] + Q[1], inc, bad)
    return cost, np.moveaxis(c, 0, 2), np.moveaxis(Shh, 0, 2)


def _confined_loglik_numpy(pos, var, frames, use, offsets, dt, D, s2, centre):
    """csrc/confined_ml.hip's mivit_track_confined_loglik restated, all ranges at once -> loglik [n] float64: NaN for a
    range without an increment and where D or s2 is not positive and finite, -inf for a rejected candidate"""
    n = len(offsets) - 1
    loglik = np.full(n, np.nan)
    rows = _ml_usable(pos, var, frames, use, offsets)
    cnt = np.array([len(r) for r in rows], np.int64)
    with np.errstate(invalid="ignore"):
        fine = (cnt >= 2) & (D > 0.0) & (D < np.inf) & (s2 > 0.0) & (s2 < np.inf)
    sel = np.nonzero(fine)[0]
    if not len(sel):
        return loglik
    sel = sel[np.argsort(-cnt[sel], kind="stable")]
    X, V, Fr = _ml_padded(rows, sel, pos, var, frames, offsets)
    cost, _, _ = _confined_cost(D[sel][:, None], s2[sel][:, None], X, V, Fr[:, 1:] - Fr[:, :-1], cnt[sel] - 1, dt,
                                None if centre is None else centre[sel][:, None, :])
    loglik[sel] = -0.5 * cost[:, 0]
    return loglik


_CF_OUTS = ("D_conf", "D_conf_std", "radius", "radius_std", "lambda", "lambda_std", "corr", "centre", "centre_std", "loglik",
            "n_increments", "status")


def _confined_ml_numpy(pos, var, frames, use, offsets, dt):
    """The arithmetic of csrc/confined_ml.hip::cf_kernel in its order (include/mivit_hip.h, mivit_track_confined_ml), all
    ranges at once -> the outputs of _CF_OUTS ([n] float64, centre and centre_std [n, 2], n_increments and status int32).
    The same Kalman recurrence, determinant by frexp, brackets, candidates, arg-min (np.argmin returns the lowest index among
    equal minima), stencil and statuses.  Differs from the kernel in expm1, exp2 and log alone."""
    n = len(offsets) - 1
    out = {k: np.full((n, 2) if k.startswith("centre") else n, np.nan) for k in _CF_OUTS[:10]}
    rows = _ml_usable(pos, var, frames, use, offsets)
    n_inc = np.array([max(len(r) - 1, 0) for r in rows], np.int32).reshape(n)
    status = np.ones(n, np.int32)
    sel = np.nonzero(n_inc >= _CF_MIN_INCREMENTS)[0]
    if not len(sel):
        return tuple(out[k] for k in _CF_OUTS[:10]) + (n_inc, status)
    sel = sel[np.argsort(-n_inc[sel], kind="stable")]
    inc = n_inc[sel].astype(np.int64)
    ns = len(sel)
    X, V, Fr = _ml_padded(rows, sel, pos, var, frames, offsets)
    d, g = X[:, 1:] - X[:, :-1], Fr[:, 1:] - Fr[:, :-1]
    rlive = np.arange(X.shape[1])[None, :] <= inc[:, None]
    with np.errstate(all="ignore"):
        D_ref = _ml_d_ref(d, g, inc, dt)
        cnt = (inc + 1).astype(np.float64)
        mean = np.cumsum(np.where(rlive[..., None], X, 0.0), axis=1)[:, -1] / cnt[:, None]
        dev = X - mean[:, None, :]
        S_ref = np.cumsum(np.where(rlive, dev[..., 0] * dev[..., 0] + dev[..., 1] * dev[..., 1], 0.0), axis=1)[:, -1] / (2.0 * cnt)
        ulo, uhi = np.full(ns, _CF_U_LO), np.full(ns, _CF_U_HI)
        wlo, whi = np.full(ns, _CF_W_LO), np.full(ns, _CF_W_HI)
        u_lo, u_hi, w_lo = (np.ones(ns, bool) for _ in range(3))
        lane = np.arange(_CF_GRID * _CF_GRID)
        li, lj = (lane >> 3).astype(np.float64), (lane & 7).astype(np.float64)
        ub, wb = np.zeros(ns), np.zeros(ns)
        for _ in range(_CF_ROUNDS):
            su, sw = (uhi - ulo) / 7.0, (whi - wlo) / 7.0
            Dj = D_ref[:, None] * np.exp2(ulo[:, None] + li[None, :] * su[:, None])
            Sj = S_ref[:, None] * np.exp2(wlo[:, None] + lj[None, :] * sw[:, None])
            best = np.argmin(_confined_cost(Dj, Sj, X, V, g, inc, dt)[0], axis=1)
            bi, bj = best >> 3, best & 7
            ub, wb = ulo + bi.astype(np.float64) * su, wlo + bj.astype(np.float64) * sw
            ulo, uhi, wlo, whi = ub - 2.0 * su, ub + 2.0 * su, wb - 2.0 * sw, wb + 2.0 * sw
            u_lo &= bi == 0
            u_hi &= bi == _CF_GRID - 1
            w_lo &= bj == 0
        Db, Sb = D_ref * np.exp2(ub), S_ref * np.exp2(wb)
        lam = Db / Sb
        st = np.where(wb >= _CF_W_HI, 2, np.where(lam * dt > _CF_FAST, 3, np.where(u_lo | u_hi | w_lo, 5, 0))).astype(np.int32)
        fD = np.array([_ML_EXP_MH, 1.0, _ML_EXP_H])
        Ds = Db[:, None] * np.repeat(fD, 3)[None, :]
        Ss = Sb[:, None] * np.tile(fD, 3)[None, :]
        c, cen, hh = _confined_cost(Ds, Ss, X, V, g, inc, dt)
        c0 = c[:, 4]
        Hdd, Hss, Hds, det, pd = _ml_hessian(c)                            # u = ln D, v = ln s2
        st = np.where(~(c0 < np.inf), 4, st).astype(np.int32)
        st = np.where(~pd & (st == 0), 4, st).astype(np.int32)
        radius = np.sqrt(2.0 * Sb)
        vl = ((Hss + Hdd) + 2.0 * Hds) / det
        full = pd & ((st == 0) | (st == 5))
        nan = np.full(ns, np.nan)
        o = {"D_conf": Db, "loglik": -0.5 * c0,
             "D_conf_std": np.where(full, Db * np.sqrt(Hss / det), nan),
             "radius": np.where(st == 2, np.inf, radius),
             "radius_std": np.where(full, (0.5 * radius) * np.sqrt(Hdd / det),
                                    np.where((st == 3) & (Hss > 0.0) & (Hss < np.inf), (0.5 * radius) / np.sqrt(Hss), nan)),
             "lambda": np.where(st == 2, 0.0, lam),
             "lambda_std": np.where(full & (vl >= 0.0), lam * np.sqrt(vl), nan),
             "corr": np.where(full, -Hds / np.sqrt(Hdd * Hss), nan)}
        keep = (st != 2)[:, None]
        o["centre"] = np.where(keep, cen[:, 4, :], np.nan)
        o["centre_std"] = np.where(keep & (st != 4)[:, None] & (hh[:, 4, :] > 0.0), 1.0 / np.sqrt(hh[:, 4, :]), np.nan)
    for k, v in o.items():
        out[k][sel] = v
    status[sel] = st
    return tuple(out[k] for k in _CF_OUTS[:10]) + (n_inc, status)


def confined_loglik(positions, offsets, D, s2, centre=None, variances=None, frames=None, use=None, dt=1.0):
    """The exact log-likelihood of every range under confined diffusion, an isotropic Ornstein-Uhlenbeck process with the
    diffusion coefficient D and the stationary variance per axis s2 = radius^2 / 2 (numbers, or one per range [n]) about a
    centre ((y, x) as [2] or [n, 2]; None: each axis takes the centre that maximises the likelihood), seen through
    localisation noise of the rows' variances: the model of estimate_confinement_ml at given parameters, to compare
    hypotheses with -> dict of the input's kind: loglik [n] float64 (NaN for a range without an increment and where D or s2
    is not positive and finite, -inf where an innovation variance is not positive).  The exposure is INSTANTANEOUS: motion
    blur is not modelled.  The other arguments are those of estimate_diffusion_ml.  CUDA tensors go to the kernel
    (csrc/confined_ml.hip), arrays and CPU tensors to the numpy restatement."""
    args = _ml_arguments(positions, offsets, variances, frames, use, dt)
    n, device = args[2].numel() - 1, args[1].device
    Dv, Sv = _ml_per_range(D, n, "D", device), _ml_per_range(s2, n, "s2", device)
    cv = None if centre is None else _ml_per_range(centre, n, "centre", device, 2)
    return _ml_dispatch(args,
                        lambda ops, pos, off, var, fr, usable: ops.track_confined_loglik(pos, off, Dv, Sv, cv, var, fr, usable, float(dt)),
                        lambda *rows: _confined_loglik_numpy(*rows, float(dt), Dv.numpy(), Sv.numpy(), None if cv is None else cv.numpy()),
                        ("loglik",))


def estimate_confinement_ml(positions, offsets, variances=None, frames=None, use=None, dt=1.0):
    """The maximum-likelihood confinement radius of every track with its standard error, and the test of whether the track
    is confined at all, from rows that each carry their own localisation variance: positions, offsets, variances, frames, use
    and dt as estimate_diffusion_ml takes them -> dict of the input's kind:
        D_conf, D_conf_std   [n] float64     the diffusion coefficient inside the well
        radius, radius_std   [n] float64     sqrt(2 s2), the RMS distance from the centre in 2-D (s2: stationary variance per axis)
        lambda, lambda_std   [n] float64     the rate D / s2 at which the particle is pulled back, per unit of dt
        corr                 [n] float64     the correlation of the estimates of ln D and ln s2
        centre, centre_std   [n, 2] float64  (y, x) of the well and its standard error at the estimates
        loglik               [n] float64     the log-likelihood at the estimates
        lr_brownian          [n] float64     2 (loglik - the loglik of estimate_diffusion_ml(..., blur=0)): the likelihood ratio
                                             against free Brownian motion, which the model nests as s2 -> inf; >= 0 up to the
                                             resolution of the search.  Its null distribution is not chi^2 (the free walk is on
                                             the boundary s2 = inf): scripts/eval_movie_accuracy.py --confined-ml prints it
        n_increments         [n] int64       the increments between usable rows
        status               [n] int64       0 fine; 1 fewer than 4 increments (NaN); 2 s2 left its first bracket upwards: the
                                             track is not confined (radius inf, lambda 0, centre and bars NaN); 3 lambda dt > 4:
                                             the particle relaxes within a frame (radius and centre stand, D_conf and lambda are
                                             lower bounds without bars); 4 the information matrix is not positive definite or no
                                             candidate was accepted (bars NaN); 5 the optimum at another end of the brackets
    The model is diffusion in a harmonic well (an isotropic Ornstein-Uhlenbeck process) seen at INSTANTANEOUS exposure (motion
    blur is not modelled) through Gaussian noise of the rows' variances, frames may be missing; its exact likelihood is a
    scalar Kalman filter per axis, conditioned on the first usable row, with the centre of each axis profiled out
    (include/mivit_hip.h has every operation).  The search is fixed: 20 rounds of an 8 x 8 grid over log2 D and log2 s2 that
    shrinks to the best candidate +- 2 cells; the bars come from the second differences of the log-likelihood with a step of
    1/64 in ln D and ln s2.  The profile likelihood UNDERESTIMATES s2 on short tracks (the centre is fitted to the same rows):
    on tracks of 100 rows that span 30 relaxation times the mean pull of ln radius is about -0.5.  CUDA tensors go to the kernel
    (csrc/confined_ml.hip: one wave per track, no limit on its length), arrays and CPU tensors to the numpy restatement, which
    differs from it in expm1, exp2 and log alone."""
    args = _ml_arguments(positions, offsets, variances, frames, use, dt)
    brownian = estimate_diffusion_ml(positions, offsets, variances, frames, use, dt, blur=0.0)["loglik"]
    out = _ml_dispatch(args, lambda ops, pos, off, var, fr, usable: ops.track_confined_ml(pos, off, var, fr, usable, float(dt)),
                       lambda *rows: _confined_ml_numpy(*rows, float(dt)), _CF_OUTS)
    with np.errstate(invalid="ignore"):                                    # arrays: -inf - -inf where no candidate was accepted
        out["lr_brownian"] = 2.0 * (out["loglik"] - brownian)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# maximum-likelihood velocity per track from rows of known variance, with error bars (csrc/directed_ml.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _directed_cost(Dc, d, g, V, inc, dt, R, given=False):
    """-2 log L of csrc/directed_ml.hip::dm_cost for the candidates Dc [n, C] of n ranges at once: d [n, >= inc[0], 2] the
    increments LESS THE SHARE OF THE VELOCITY THE RECURRENCE RUNS ABOUT (the unweighted one, or the caller's), g [n, >=
    inc[0]] their gaps in frames, V [n, >= inc[0] + 1, 2] the row variances, inc [n] >= 1 the increments of each range IN
    DESCENDING ORDER; given: the quadratic form is A (the velocity stands), else A - B B / C (the velocity is profiled) ->
    (cost [n, C], B / C [n, C, 2] what the profiled velocity adds to the one d was taken about, C [n, C, 2]).  Elementwise
    the kernel's operations in its order (include/mivit_hip.h, mivit_track_directed_ml); the two differ in log alone."""
    n, C = Dc.shape
    c1 = (2.0 * Dc) * dt
    cR, tR = R * c1, 2.0 * R
    pm, pe = np.full((n, C), 0.5), np.ones((n, C), np.int64)
    bad = np.zeros((n, C), bool)
    rinv, z, w = np.zeros((2, n, C)), np.zeros((2, n, C)), np.zeros((2, n, C))
    A, B, Cc = np.zeros((2, n, C)), np.zeros((2, n, C)), np.zeros((2, n, C))
    with np.errstate(all="ignore"):
        for k in range(int(inc[0]) if n else 0):
            na = int(np.count_nonzero(inc > k))
            gk = g[:na, k].astype(np.float64)
            base = c1[:na] * (gk - tR)[:, None]
            m = (gk * dt)[:, None]
            for ax in (0, 1):
                pv, v, dd = V[:na, k, ax][:, None], V[:na, k + 1, ax][:, None], d[:na, k, ax][:, None]
                a = (base + pv) + v
                if k == 0:
                    e, zz, ww = a, np.broadcast_to(dd, a.shape), np.broadcast_to(m, a.shape)
                else:
                    b = cR[:na] - pv
                    l = b * rinv[ax, :na]
                    e = a - l * b
                    zz = dd - l * z[ax, :na]
                    ww = m - l * w[ax, :na]
                bad[:na] |= ~(e > 0.0)
                r = 1.0 / e
                A[ax, :na] = A[ax, :na] + (zz * zz) * r
                B[ax, :na] = B[ax, :na] + (zz * ww) * r
                Cc[ax, :na] = Cc[ax, :na] + (ww * ww) * r
                _ml_prod_mul(pm, pe, e)
                rinv[ax, :na], z[ax, :na], w[ax, :na] = r, zz, ww
        bad |= ~((Cc[0] > 0.0) & (Cc[0] < np.inf) & (Cc[1] > 0.0) & (Cc[1] < np.inf))
        Q = A[0] + A[1] if given else (A[0] - (B[0] * B[0]) / Cc[0]) + (A[1] - (B[1] * B[1]) / Cc[1])
        cost = _ml_finish_cost(pm, pe, Q, inc, bad)
        return cost, np.moveaxis(B / Cc, 0, 2), np.moveaxis(Cc, 0, 2)


def _directed_rows(pos, var, frames, offsets, rows, sel, inc, dt, velocity=None):
    """What the two restatements of csrc/directed_ml.hip share: the padded rows of the ranges sel -> (d [ns, M, 2] the
    increments less the velocity's share, the velocity being `velocity` [ns, 2] or, where None, the unweighted one (last
    usable position - first) / (G dt) of dm_start; g [ns, M] the gaps; V the variances; that velocity [ns, 2])"""
    X, V, Fr = _ml_padded(rows, sel, pos, var, frames, offsets)
    g = Fr[:, 1:] - Fr[:, :-1]
    live = np.arange(g.shape[1])[None, :] < inc[:, None]
    with np.errstate(all="ignore"):
        if velocity is None:
            T = np.where(live, g, 0).sum(axis=1).astype(np.float64) * dt
            velocity = (X[np.arange(len(sel)), inc] - X[:, 0]) / T[:, None]
        m = g.astype(np.float64) * dt
        d = (X[:, 1:] - X[:, :-1]) - velocity[:, None, :] * m[:, :, None]
    return d, g, V, velocity


def _directed_ml_numpy(pos, var, frames, use, offsets, dt, R):
    """The arithmetic of csrc/directed_ml.hip::dm_kernel in its order (include/mivit_hip.h, mivit_track_directed_ml), all
    ranges at once: the arguments of _diffusion_ml_numpy -> (D, D_std [n] float64, velocity, velocity_std [n, 2] float64,
    loglik [n] float64, n_increments, status [n] int32).  The same two recurrences, three sums, determinant by frexp and
    search; np.argmin returns the lowest index among equal minima.  Differs from the kernel in log and exp2 alone."""
    n = len(offsets) - 1
    D, D_std, loglik = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    vel, vel_std = np.full((n, 2), np.nan), np.full((n, 2), np.nan)
    status = np.ones(n, np.int32)
    rows = _ml_usable(pos, var, frames, use, offsets)
    n_inc = np.array([max(len(r) - 1, 0) for r in rows], np.int32).reshape(n)
    sel = np.nonzero(n_inc >= 2)[0]
    if not len(sel):
        return D, D_std, vel, vel_std, loglik, n_inc, status
    sel = sel[np.argsort(-n_inc[sel], kind="stable")]                      # descending: the ranges still running are a prefix
    inc = n_inc[sel].astype(np.int64)
    ns = len(sel)
    d, g, V, u0 = _directed_rows(pos, var, frames, offsets, rows, sel, inc, dt)
    with np.errstate(all="ignore"):
        D_ref = _ml_d_ref(d, g, inc, dt)
        lo, hi = np.full(ns, _ML_U_LO), np.full(ns, _ML_U_HI)
        all_lo, all_hi = np.ones(ns, bool), np.ones(ns, bool)
        lane, each = np.arange(_ML_CANDIDATES, dtype=np.float64), np.arange(ns)
        Db = np.zeros(ns)
        for _ in range(_ML_ROUNDS):
            step = (hi - lo) / 63.0
            Dj = D_ref[:, None] * np.exp2(lo[:, None] + lane[None, :] * step[:, None])
            j = np.argmin(_directed_cost(Dj, d, g, V, inc, dt, R)[0], axis=1)
            all_lo &= j == 0
            all_hi &= j == _ML_CANDIDATES - 1
            Db = Dj[each, j]
            jl, jh = np.maximum(j - 1, 0), np.minimum(j + 1, _ML_CANDIDATES - 1)
            lo, hi = lo + jl.astype(np.float64) * step, lo + jh.astype(np.float64) * step
        st = np.where(all_lo, 2, np.where(all_hi, 3, 0)).astype(np.int32)
        Db = np.where(all_lo, 0.0, Db)
        c, bc, Cc = _directed_cost(np.stack([Db, Db * _ML_EXP_H, Db * _ML_EXP_MH], axis=1), d, g, V, inc, dt, R)
        info = _ml_curvature(c[:, 1], c[:, 0], c[:, 2])
        curved = (info > 0.0) & (info < np.inf)
        fine = (c[:, 0] < np.inf)[:, None]
        D[sel], loglik[sel] = Db, -0.5 * c[:, 0]
        D_std[sel] = np.where(curved & (st != 2), Db / np.sqrt(info), np.nan)
        vel[sel] = np.where(fine, u0 + bc[:, 0, :], np.nan)
        vel_std[sel] = np.where(fine, 1.0 / np.sqrt(Cc[:, 0, :]), np.nan)
        status[sel] = np.where(~curved & (st == 0), 4, st)
    return D, D_std, vel, vel_std, loglik, n_inc, status


def _directed_loglik_numpy(pos, var, frames, use, offsets, dt, R, D, velocity):
    """csrc/directed_ml.hip's mivit_track_directed_loglik restated, all ranges at once -> (loglik [n], velocity [n, 2],
    velocity_std [n, 2]) float64: loglik NaN for a range without an increment and where D is negative or not finite or a
    given velocity is not finite, -inf for a rejected candidate; the velocity of the fit and its standard error, NaN where
    loglik is not finite"""
    n = len(offsets) - 1
    loglik, vel, vel_std = np.full(n, np.nan), np.full((n, 2), np.nan), np.full((n, 2), np.nan)
    rows = _ml_usable(pos, var, frames, use, offsets)
    cnt = np.array([len(r) for r in rows], np.int64)
    with np.errstate(invalid="ignore"):
        fine = (cnt >= 2) & (D >= 0.0) & (D < np.inf)
        if velocity is not None:
            fine &= np.isfinite(velocity).all(axis=1)
    sel = np.nonzero(fine)[0]
    if not len(sel):
        return loglik, vel, vel_std
    sel = sel[np.argsort(-cnt[sel], kind="stable")]
    inc = cnt[sel] - 1
    d, g, V, u = _directed_rows(pos, var, frames, offsets, rows, sel, inc, dt, None if velocity is None else velocity[sel])
    cost, bc, Cc = _directed_cost(D[sel][:, None], d, g, V, inc, dt, R, given=velocity is not None)
    with np.errstate(all="ignore"):
        has = (cost[:, 0] < np.inf)[:, None]
        loglik[sel] = -0.5 * cost[:, 0]
        vel[sel] = np.where(has, u + bc[:, 0, :], np.nan)
        vel_std[sel] = np.where(has, 1.0 / np.sqrt(Cc[:, 0, :]), np.nan)
    return loglik, vel, vel_std


def _check_blur(blur):
    if not 0.0 <= float(blur) <= 0.25:
        raise ValueError(f"blur must lie in [0, 1/4], got {blur}")


def directed_loglik(positions, offsets, D, velocity=None, variances=None, frames=None, use=None, dt=1.0, blur=0.0):
    """The exact log-likelihood of every range under directed motion: diffusion with the coefficient D (a number, or one per
    range [n]) plus a constant velocity ((y, x) in pixels per unit of dt as [2] or [n, 2]; None: each axis takes the velocity
    that maximises the likelihood), seen through localisation noise of the rows' variances and motion blur: the model of
    estimate_directed_ml at given parameters, to compare hypotheses with -> dict of the input's kind: loglik [n] float64 (NaN
    for a range without an increment and where D is negative or not finite or a given velocity is not finite, -inf where the
    covariance is not positive definite), and with velocity=None also velocity [n, 2] and velocity_std [n, 2], the profiled
    velocity and its standard error at that D.  With velocity 0 it is the likelihood of estimate_diffusion_ml at D.  The
    other arguments are those of estimate_diffusion_ml.  CUDA tensors go to the kernel (csrc/directed_ml.hip), arrays and
    CPU tensors to the numpy restatement."""
    _check_blur(blur)
    args = _ml_arguments(positions, offsets, variances, frames, use, dt)
    n, device = args[2].numel() - 1, args[1].device
    Dv = _ml_per_range(D, n, "D", device)
    vv = None if velocity is None else _ml_per_range(velocity, n, "velocity", device, 2)
    keys = ("loglik", "velocity", "velocity_std") if vv is None else ("loglik",)

    def restated(*rows):
        got = _directed_loglik_numpy(*rows, float(dt), float(blur), Dv.numpy(), None if vv is None else vv.numpy())
        return got if vv is None else got[0]

    return _ml_dispatch(args, lambda ops, pos, off, var, fr, usable: ops.track_directed_loglik(pos, off, Dv, vv, var, fr, usable,
                                                                                                float(dt), float(blur)),
                        restated, keys)


_DM_OUTS = ("D_dir", "D_dir_std", "velocity", "velocity_std", "loglik", "n_increments", "status")


def estimate_directed_ml(positions, offsets, variances=None, frames=None, use=None, dt=1.0, blur=0.0):
    """The maximum-likelihood velocity of every track with its standard error, and the test of whether the track is directed
    at all, from rows that each carry their own localisation variance: positions, offsets, variances, frames, use, dt and
    blur as estimate_diffusion_ml takes them -> dict of the input's kind:
        D_dir, D_dir_std        [n] float64     the diffusion coefficient about the directed path; 0 at status 2
        velocity, velocity_std  [n, 2] float64  (y, x) in pixels per unit of dt, and its standard error 1 / sqrt(C) at D_dir
        speed, speed_std        [n] float64     |velocity| and its standard error by the delta method, sqrt(vy^2 sy^2 + vx^2
                                                sx^2) / speed (NaN at speed 0)
        loglik                  [n] float64     the log-likelihood at the estimates
        lr_brownian             [n] float64     2 (loglik - the loglik of estimate_diffusion_ml(..., blur=blur)): the likelihood
                                                ratio against free diffusion, which the model nests at velocity 0; >= 0 up to
                                                the resolution of the searches
        p_brownian              [n] float64     exp(-lr_brownian / 2), the chi^2 survival function at 2 degrees of freedom: 1
                                                where lr_brownian <= 0, NaN where either fit has status 1
        n_increments            [n] int64       the increments between usable rows
        status                  [n] int64       0 fine; 1 fewer than 2 increments (NaN); 2 the minimum at the lower end of the
                                                search: the track is a straight line within its noise (D_dir 0, D_dir_std NaN;
                                                velocity and velocity_std stand where the likelihood at D = 0 is finite); 3 at
                                                its upper end; 4 the curvature is not positive (D_dir_std NaN)
    The increments of a track are Gaussian with the tridiagonal covariance of estimate_diffusion_ml about velocity * gap *
    dt (an exposure average shifts every row of a constant-velocity track alike, so blur leaves the mean alone).  The
    velocity enters linearly and is profiled out in closed form inside the LDL^T recurrence: a second recurrence on the
    regressor gap * dt and three sums per axis, u = B / C with the variance 1 / C at fixed D; mean and covariance parameters
    of a Gaussian share no Fisher information, so these are the bars at D_dir, and D_dir_std comes from the curvature of the
    profile likelihood in ln D.  The search is that of estimate_diffusion_ml, about a D_ref taken from the residuals about the
    unweighted velocity (last usable position - first) / elapsed time, so that a velocity added to a track changes the
    velocity by that much and nothing else (include/mivit_hip.h has every operation).  This is plain maximum likelihood, not
    REML, so that lr_brownian compares nested models on the same data: D_dir is low by about one part in n_increments (the
    velocity is fitted to the same rows), a mean pull of ln D of about -0.27 on tracks of 100 rows.  estimate_drift removes
    whatever velocity all tracks share; what this fit sees after it is each track's own.  CUDA tensors go to the kernel
    (csrc/directed_ml.hip: one wave per track, no limit on its length), arrays and CPU tensors to the numpy restatement,
    which differs from it in log and exp2 alone."""
    _check_blur(blur)
    args = _ml_arguments(positions, offsets, variances, frames, use, dt)
    free = estimate_diffusion_ml(positions, offsets, variances, frames, use, dt, blur=blur)
    out = _ml_dispatch(args, lambda ops, pos, off, var, fr, usable: ops.track_directed_ml(pos, off, var, fr, usable, float(dt),
                                                                                         float(blur)),
                       lambda *rows: _directed_ml_numpy(*rows, float(dt), float(blur)), _DM_OUTS)
    xp = torch if args[0] else np
    v, s = out["velocity"], out["velocity_std"]
    with np.errstate(invalid="ignore", divide="ignore"):                   # arrays: 0 / 0 at speed 0, -inf - -inf
        out["speed"] = xp.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
        out["speed_std"] = xp.sqrt((v[:, 0] * v[:, 0]) * (s[:, 0] * s[:, 0]) + (v[:, 1] * v[:, 1]) * (s[:, 1] * s[:, 1])) / out["speed"]
        out["lr_brownian"] = 2.0 * (out["loglik"] - free["loglik"])
        out["p_brownian"] = xp.exp(-0.5 * out["lr_brownian"].clip(min=0.0))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# run-and-pause transport: changepoints of the velocity and one row of estimates per stretch (csrc/segment.hip)
# ----------------------------------------------------------------------------------------------------------------------
_TRANSPORT_CLASSES = {"both": 0, "directed": 1, "diffusive": 2}


def _transport_numpy(pos, offsets, min_len, penalty, velocity_penalty, min_var, classes, return_margin=False):
    """The arithmetic of csrc/segment.hip::partition_kernel<TransportModel> in its order (include/mivit_hip.h, mivit_segment_transport):
    np.cumsum is the sequential prefix sum, np.argmin returns the lowest index among equal minima.  pos [N, 2] float64,
    offsets [n_tracks + 1] int64, classes 0 (both), 1 (directed) or 2 (diffusive) -> (seg_start [N] int32, seg_class [N]
    int32, cost [n_tracks] float64).  Differs from the kernel in log alone.  return_margin: also margin [n_tracks], the smallest
    over the backtracked path of two gaps: between the chosen candidate and the runner-up, and (classes 0) |C0 - C1| at the
    chosen candidate -- a class flip is as much a change of the answer as a moved cut.  inf where neither exists."""
    n_tracks = len(offsets) - 1
    seg_start = np.zeros(len(pos), np.int32)
    seg_class = np.zeros(len(pos), np.int32)
    cost = np.full(n_tracks, np.nan)
    margin = np.full(n_tracks, np.inf)
    for k in range(n_tracks):
        a, b = int(offsets[k]), int(offsets[k + 1])
        L = b - a
        if L >= 1:
            seg_start[a] = 1
        Linc = L - 1
        if Linc < 1:
            continue
        p = pos[a:b]
        dy, dx = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
        cs2 = np.concatenate([np.zeros(1), np.cumsum(dy * dy + dx * dx)])
        csy = np.concatenate([np.zeros(1), np.cumsum(dy)])
        csx = np.concatenate([np.zeros(1), np.cumsum(dx)])
        lg = np.log(float(Linc))
        beta, gamma = penalty * lg, velocity_penalty * lg

        def step(j, cand):
            n = (j - cand).astype(np.float64)
            tn = 2.0 * n
            SS, Sy, Sx = cs2[j] - cs2[cand], csy[j] - csy[cand], csx[j] - csx[cand]
            with np.errstate(divide="ignore", invalid="ignore"):
                C0 = tn * np.log(np.maximum(SS / tn, min_var))
                C1 = tn * np.log(np.maximum((SS - (Sy * Sy + Sx * Sx) / n) / tn, min_var)) + gamma
                if classes == 1:
                    cls, C, flip = np.ones(len(cand), np.int32), C1, np.full(len(cand), np.inf)
                elif classes == 2:
                    cls, C, flip = np.zeros(len(cand), np.int32), C0, np.full(len(cand), np.inf)
                else:
                    pick = C1 < C0
                    cls, C, flip = pick.astype(np.int32), np.where(pick, C1, C0), np.abs(C0 - C1)
                return (F[cand] + C) + beta, cls, flip

        F = np.full(Linc + 1, np.nan)
        F[0] = -beta
        prev = np.zeros(Linc + 1, np.int64)
        pcls = np.zeros(Linc + 1, np.int32)
        gap = np.full(Linc + 1, np.inf)
        if Linc < min_len:
            v, cls, flip = step(Linc, np.zeros(1, np.int64))
            F[Linc], pcls[Linc], gap[Linc] = v[0], cls[0], flip[0]
        for j in range(min_len, Linc + 1):
            cand = np.concatenate([np.zeros(1, np.int64), np.arange(min_len, j - min_len + 1, dtype=np.int64)])
            v, cls, flip = step(j, cand)
            if np.isnan(v).all():
                F[j] = v[0]
                continue
            m = int(np.argmin(v))
            F[j], prev[j], pcls[j] = v[m], cand[m], cls[m]
            if return_margin:
                gap[j] = min(flip[m], np.partition(v, 1)[1] - v[m]) if len(v) > 1 else flip[m]
        cost[k] = F[Linc]
        j = Linc
        while j > 0:
            margin[k] = min(margin[k], gap[j])
            i = int(prev[j])
            seg_class[a + i:a + (L if j == Linc else j)] = pcls[j]
            if i > 0:
                seg_start[a + i] = 1
            j = i
    return (seg_start, seg_class, cost, margin) if return_margin else (seg_start, seg_class, cost)


def _transport_stats_numpy(pos, seg_offsets, seg_track_end, dt, blur):
    """The arithmetic of csrc/segment.hip::stretch_stats_kernel<true> in its order: np.cumsum(...)[-1] is a sequential sum.  ->
    (velocity [n_seg, 2], D_res, D_cve, sigma2 [n_seg] float64, n_increments [n_seg] int32), bitwise the kernel's."""
    n_seg = len(seg_track_end)
    velocity = np.full((n_seg, 2), np.nan)
    d_res, d_cve, sigma2 = np.full(n_seg, np.nan), np.full(n_seg, np.nan), np.full(n_seg, np.nan)
    n_inc = np.zeros(n_seg, np.int32)
    R = float(blur)
    for s in range(n_seg):
        r0 = max(int(seg_offsets[s]), 0)
        r1 = min(int(seg_offsets[s + 1]), int(seg_track_end[s]) - 1, len(pos) - 1)
        n = max(r1 - r0, 0)
        n_inc[s] = n
        if n < 1:
            continue
        p = pos[r0:r1 + 1]
        dy, dx = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
        my, mx = np.cumsum(dy)[-1] / float(n), np.cumsum(dx)[-1] / float(n)
        velocity[s, 0], velocity[s, 1] = my / dt, mx / dt
        ey, ex = dy - my, dx - mx
        S2 = np.cumsum(ey * ey + ex * ex)[-1]
        d_res[s] = S2 / ((4.0 * float(n)) * dt)
        if n >= 2:
            S11 = np.cumsum(ey[:-1] * ey[1:] + ex[:-1] * ex[1:])[-1]
            m1 = 2.0 * float(n - 1)
            d_cve[s] = d_res[s] + S11 / (m1 * dt)
            sigma2[s] = (R * S2) / (2.0 * float(n)) + ((2.0 * R - 1.0) * S11) / m1
    return velocity, d_res, d_cve, sigma2, n_inc


def segment_transport(positions, offsets, dt=1.0, min_len=4, penalty=3.0, velocity_penalty=3.0, min_var=1e-12, classes="both",
                      blur=0.0):
    """Tracks whose velocity changes (run and pause): the optimal partition of every track into stretches that are each
    diffusive (class 0: zero-mean increments of one variance) or directed (class 1: one variance about a constant velocity),
    and the estimates of each stretch about its own velocity.  positions, offsets, dt, min_len, penalty, min_var and blur as
    segment_tracks takes them -> dict:
        seg_offsets [n_seg + 1] int64, seg_track [n_seg] int64      as segment_tracks returns them
        seg_class   [n_seg] int64       0 diffusive, 1 directed
        velocity    [n_seg, 2] float64  the mean increment / dt as (y, x), whatever the class; speed [n_seg] its length
        D_res       [n_seg] float64     the maximum-likelihood D about that velocity, without localisation noise
        D_cve, sigma2 [n_seg] float64   Vestergaard's estimators on the increments minus their mean: noise and blur cancel
        n_increments [n_seg] int64, cost [n_tracks] float64
    Penalised likelihood as in segment_tracks, with two models per stretch: a directed stretch pays gamma = velocity_penalty *
    log(increments of the track) for its two velocity components on top of beta per changepoint, and a stretch is directed
    only where that is strictly cheaper.  classes "directed" gives every stretch a velocity, "diffusive" none (the partition
    and cost of segment_tracks bit for bit).  A whole-track fit (estimate_directed_ml) averages a run with a pause; pass
    seg_offsets to it, or to estimate_diffusion_ml, for the per-stretch fits with error bars.  include/mivit_hip.h has the
    arithmetic.  CUDA tensors go to the kernels (csrc/segment.hip: two launches; a track has at most ops.TRANSPORT_MAX_LEN
    rows), numpy arrays and CPU tensors to the numpy restatements; the output is of the input's kind."""
    if not float(velocity_penalty) >= 0.0:
        raise ValueError(f"velocity_penalty must be >= 0, got {velocity_penalty}")
    if not isinstance(classes, str) or classes not in _TRANSPORT_CLASSES:
        raise ValueError(f"classes must be one of {', '.join(_TRANSPORT_CLASSES)}, got {classes!r}")
    offsets = _check_partition_args(positions, offsets, dt, min_len, penalty, min_var, blur, "TRANSPORT_MAX_LEN")
    min_len, penalty, velocity_penalty, min_var = int(min_len), float(penalty), float(velocity_penalty), float(min_var)
    dt, blur = float(dt), float(blur)
    is_t = torch.is_tensor(positions)
    if is_t and positions.device.type == "cuda":
        from .. import ops
        pos = positions.detach().double().contiguous()
        seg_start, row_class, cost = ops.segment_transport(pos, offsets.int().contiguous(), min_len, penalty, velocity_penalty,
                                                           min_var, classes)
        first, seg_offsets, seg_track, track_end = _stretch_layout(seg_start, offsets.long().contiguous(), pos.shape[0])
        velocity, d_res, d_cve, sigma2, n_inc = ops.transport_stats(pos, seg_offsets.int(), track_end.int(), dt, blur)
        return {"seg_offsets": seg_offsets, "seg_track": seg_track, "seg_class": row_class[first].long(), "velocity": velocity,
                "speed": torch.sqrt(velocity[:, 0] * velocity[:, 0] + velocity[:, 1] * velocity[:, 1]), "D_res": d_res,
                "D_cve": d_cve, "sigma2": sigma2, "n_increments": n_inc.long(), "cost": cost}
    pos = positions.detach().double().numpy() if is_t else np.asarray(positions, dtype=np.float64)
    off = (offsets.detach().numpy() if is_t else offsets).astype(np.int64)
    seg_start, row_class, cost = _transport_numpy(pos, off, min_len, penalty, velocity_penalty, min_var, _TRANSPORT_CLASSES[classes])
    first, seg_offsets, seg_track, track_end = _stretch_layout(seg_start, off, len(pos))
    velocity, d_res, d_cve, sigma2, n_inc = _transport_stats_numpy(pos, seg_offsets, track_end, dt, blur)
    out = {"seg_offsets": seg_offsets, "seg_track": seg_track, "seg_class": row_class[first].astype(np.int64), "velocity": velocity,
           "speed": np.sqrt(velocity[:, 0] * velocity[:, 0] + velocity[:, 1] * velocity[:, 1]), "D_res": d_res, "D_cve": d_cve,
           "sigma2": sigma2, "n_increments": n_inc.astype(np.int64), "cost": cost}
    return {k: torch.from_numpy(v) for k, v in out.items()} if is_t else out
