"""CPU: the numpy restatement of the real-movie front end (helpers/tracking.py) and helpers/msd.py against the reference's
recorded outputs (tests/golden/tracking/tracking.npz, written by tests/golden/make_tracking_golden.py from the real
reference), plus the argument checks.  The bars and their origin are in tests/tracking_common.py."""
import os
import pickle

import numpy as np
import pytest
import torch

import tracking_common as tc
from moleculardiffusion_mivit_amd.helpers import msd as M
from moleculardiffusion_mivit_amd.helpers import tracking as T


@pytest.fixture(scope="module")
def gold():
    return np.load(tc.GOLDEN)


@pytest.fixture(scope="module")
def tracked():
    return {name: T.track_particles(tc.movie(name), min_track_length=5) for name in tc.MOVIES}


def _tracks_array(tracks):
    return np.array([(tid, fr, y, x) for tid, pos in tracks.items() for fr, y, x in pos], np.int64)


def test_fixture_was_made_with_this_numpy_major(gold):
    """threshold_percentage * max(dog) is one float32 product under numpy 2's promotion rules, which the fixture relies on."""
    assert str(gold["numpy_version"]).split(".")[0] == np.__version__.split(".")[0] == "2"


def test_gaussian_half_kernel_is_scipys():
    from scipy.ndimage import _filters
    for sigma in (0.5, 1.0, 1.3, 2.0, 3.7):
        r = int(4.0 * sigma + 0.5)
        want = _filters._gaussian_kernel1d(sigma, 0, r)
        got = T.gaussian_half_kernel(sigma)
        assert len(got) == r + 1 and np.array_equal(got, want[r:]) and np.array_equal(got, want[r::-1])


def test_dog_restatement_is_bitwise_scipy():
    from scipy import ndimage
    rng = np.random.default_rng(99)
    frames = np.concatenate([rng.poisson(50.0, (20, 40, 57)).astype(np.float32),
                             rng.normal(0, 1e3, (20, 40, 57)).astype(np.float32)])
    for s1, s2 in ((1.0, 2.0), (0.7, 1.9), (1.5, 4.0)):
        got = T._dog_numpy(frames, T.gaussian_half_kernel(s1), T.gaussian_half_kernel(s2))
        for f in range(len(frames)):
            want = ndimage.gaussian_filter(frames[f], sigma=s1) - ndimage.gaussian_filter(frames[f], sigma=s2)
            assert np.array_equal(got[f], want), (s1, s2, f)          # DOG_BAR_ULP = 0
    assert tc.DOG_BAR_ULP == 0


@pytest.mark.parametrize("name", list(tc.MOVIES))
def test_peaks_per_frame_same_coordinates_same_order(gold, name):
    coords, dog = T.detect_particles_movie(tc.movie(name))
    assert [len(c) for c in coords] == list(gold[f"{name}_peak_counts"])
    assert np.array_equal(np.concatenate(coords), gold[f"{name}_peaks"])
    assert coords[0].dtype == np.int64 and dog.dtype == np.float32
    assert np.array_equal(dog[gold[f"{name}_dog_frames"]], gold[f"{name}_dog"])
    # the single-frame entry point of the reference
    c0, d0 = T.detect_particles(tc.movie(name)[0])
    assert np.array_equal(c0, coords[0]) and np.array_equal(d0, dog[0])


@pytest.mark.parametrize("min_distance", [1, 2, 3, 4, 5])
def test_peaks_match_the_peak_local_max_statement(min_distance):
    mov = tc.movie("odd")[:3]
    coords, dog = T.detect_particles_movie(mov, min_distance=min_distance, threshold_percentage=0.05)
    for f in range(len(mov)):
        want = tc.peak_local_max(dog[f], min_distance=min_distance, threshold_abs=np.float32(0.05) * dog[f].max(),
                                 exclude_border=False)
        assert np.array_equal(coords[f], want)


def test_flat_and_empty_frames_have_no_peak():
    mov = np.full((2, 40, 40), 7.0, np.float32)
    coords, _ = T.detect_particles_movie(mov)
    assert all(c.shape == (0, 2) for c in coords)
    tracks, det, _ = T.track_particles(mov)
    assert tracks == {} and len(det) == 0 and list(det.columns) == ["frame", "y", "x", "track_id"]


@pytest.mark.parametrize("name", list(tc.MOVIES))
def test_tracks_and_detections_equal(gold, tracked, name):
    tracks, det, dog = tracked[name]
    assert np.array_equal(_tracks_array(tracks), gold[f"{name}_tracks"])
    assert list(tracks) == list(range(len(tracks)))
    assert list(det.columns) == ["frame", "y", "x", "track_id"]
    for col in det.columns:
        assert det[col].dtype == gold[f"{name}_det_{col}"].dtype and np.array_equal(det[col].to_numpy(), gold[f"{name}_det_{col}"])
    assert len(dog) == len(tc.movie(name))


def test_link_particles_matches_the_loop_statement():
    rng = np.random.default_rng(1)
    c0, c1 = rng.integers(0, 60, (9, 2)), rng.integers(0, 60, (7, 2))
    links, u0, u1 = T.link_particles(c0, c1, max_distance=15)
    from scipy.optimize import linear_sum_assignment
    cost = np.array([[np.sqrt(((a - b) ** 2).sum()) for b in c1] for a in c0])
    r, c = linear_sum_assignment(cost)
    want = [(i, j) for i, j in zip(r, c) if cost[i, j] <= 15]
    assert links == want
    assert u0 == [i for i in range(9) if i not in dict(want)] and u1 == [j for j in range(7) if j not in {b for _, b in want}]
    assert T.link_particles(np.zeros((0, 2)), c1) == ([], [], list(range(7)))
    assert T.link_particles(c0, np.zeros((0, 2))) == ([], list(range(9)), [])


@pytest.mark.parametrize("name", list(tc.MOVIES))
def test_dataframe_columns_index_and_fit(gold, tracked, name):
    mov = tc.movie(name)
    tracks = tracked[name][0]
    patches = T.extract_particle_patches(mov, tracks, patch_size=tc.PATCH_SIZE)
    df = T.tracks_to_dataframe(tracks, patches, tc.PATCH_SIZE)
    assert list(df.columns) == [str(c) for c in gold[f"{name}_df_columns"]]
    assert list(df.index.names) == ["track_id", "frame"]
    assert np.array_equal(np.array(list(df.index), np.int64), gold[f"{name}_df_index"])
    for col in ("nbr_frames", "x", "y", "max_intensity", "max_intensity_over_track", "mean_max_intensity_over_track",
                "std_max_intensity_over_track"):
        want = gold[f"{name}_df_{col}"]
        assert df[col].dtype == want.dtype and np.array_equal(df[col].to_numpy(), want), col
    bars = {"x_refined": tc.FIT_BAR["x0"], "y_refined": tc.FIT_BAR["y0"], "psf_size": tc.FIT_BAR["sigma"]}
    for col, bar in bars.items():
        err = np.abs(df[col].to_numpy() - gold[f"{name}_df_{col}"]).max()
        print(f"{name} {col}: max |restatement - reference| {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (col, err, bar)
    # the displacement columns follow from the refined positions: two positions, each within its bar
    step_bar = 2 * np.hypot(tc.FIT_BAR["x0"], tc.FIT_BAR["y0"])
    assert np.abs(df["displacement"].to_numpy() - gold[f"{name}_df_displacement"]).max() <= step_bar
    assert np.abs(df["mean_displacement"].to_numpy() - gold[f"{name}_df_mean_displacement"]).max() <= step_bar
    assert np.abs(df["mean_psf_size"].to_numpy() - gold[f"{name}_df_mean_psf_size"]).max() <= tc.FIT_BAR["sigma"]


def test_flat_path_equals_the_dataframe_path(tracked):
    mov = tc.movie("odd")
    tracks = tracked["odd"][0]
    rows = np.array([(fr, y, x) for pos in tracks.values() for fr, y, x in pos])
    flat = T.extract_patches_flat(mov, rows[:, 0], rows[:, 1], rows[:, 2], tc.PATCH_SIZE)
    per_track = T.extract_particle_patches(mov, tracks, patch_size=tc.PATCH_SIZE)
    assert np.array_equal(flat, np.concatenate([per_track[t] for t in tracks]))
    res = T.refine_localizations(flat, rows[:, 1], rows[:, 2])
    df = T.tracks_to_dataframe(tracks, per_track, tc.PATCH_SIZE)
    keys = [(tid, fr) for tid, pos in tracks.items() for fr, _, _ in pos]
    assert np.array_equal(res["x_refined"], df.loc[keys, "x_refined"].to_numpy())
    assert np.array_equal(res["psf_size"], df.loc[keys, "psf_size"].to_numpy())
    assert (res["status"] == 0).all()


def test_fit_recovers_a_noise_free_spot_and_falls_back_on_failure():
    P = 9
    ax = np.arange(P, dtype=np.float64)
    x, y = np.meshgrid(ax, ax)
    truth = np.array([150.0, 4.3, 3.6, 1.25, 12.0])
    patch = (truth[4] + truth[0] * np.exp(-((x - truth[1]) ** 2 + (y - truth[2]) ** 2) / (2 * truth[3] ** 2)))
    p, peak, status = T._refine_numpy(patch[None])                   # float64 patch: exact model
    assert status[0] == 0 and np.abs(p[0] - truth).max() < 1e-9
    assert peak[0] == patch.max()
    bad = np.full((1, P, P), np.nan, np.float32)
    res = T.refine_localizations(np.concatenate([patch[None].astype(np.float32), bad]), np.array([20, 31]), np.array([40, 52]))
    assert res["status"][0] == 0 and res["status"][1] != 0
    assert res["x_refined"][1] == 52 and res["y_refined"][1] == 31 and res["psf_size"][1] == 10
    assert abs(res["x_refined"][0] - (40 - 4 + 4.3)) < 1e-5


def test_pure_noise_patches_give_finite_numbers_and_a_status():
    rng = np.random.default_rng(0)
    p, peak, status = T._refine_numpy(rng.poisson(20.0, (64, 7, 7)).astype(np.float32))
    assert np.isfinite(p).all() and np.isfinite(peak).all() and set(status) <= {0, 1, 2}


def test_msd_functions_agree_with_the_reference(gold):
    traj, t = gold["msd_traj"], gold["msd_time"]
    msd = M.mean_square_displacements(traj)
    assert np.array_equal(msd, gold["msd"])
    assert np.array_equal(M.estimateDfromMSDs(msd, t), gold["msd_D"])
    assert np.array_equal(M.estimateDfromMSDsWeighted(msd, t), gold["msd_D_weighted"])
    tm = M.mean_square_displacements(torch.from_numpy(traj))
    assert torch.is_tensor(tm) and np.allclose(tm.numpy(), gold["msd"], rtol=1e-12, atol=0)
    assert np.allclose(M.estimateDfromMSDs(tm, t).numpy(), gold["msd_D"], rtol=1e-10)
    assert np.allclose(M.estimateDfromMSDsWeighted(tm, t).numpy(), gold["msd_D_weighted"], rtol=1e-12)


def test_argument_errors():
    mov = tc.movie("odd")[:2]
    with pytest.raises(ValueError, match="F, H, W"):
        T.detect_particles_movie(mov[0])
    with pytest.raises(ValueError, match="H, W"):
        T.detect_particles(mov)
    with pytest.raises(ValueError, match="sigma1 <= sigma2"):
        T.detect_particles_movie(mov, sigma1=2.0, sigma2=1.0)
    with pytest.raises(ValueError, match="min_distance"):
        T.detect_particles_movie(mov, min_distance=0)
    with pytest.raises(ValueError, match="filter radius"):
        T.detect_particles_movie(mov[:, :8, :], sigma2=2.0)
    with pytest.raises(ValueError, match="radius of 20"):
        T.detect_particles_movie(mov, sigma2=5.0)
    with pytest.raises(ValueError, match="odd"):
        T.extract_patches_flat(mov, [0], [5], [5], patch_size=8)
    with pytest.raises(ValueError, match="odd and from 3 to 15"):
        T.refine_gaussian_patches(np.zeros((1, 17, 17), np.float32))
    with pytest.raises(ValueError, match="N, P, P"):
        T.refine_gaussian_patches(np.zeros((1, 7, 9), np.float32))
    with pytest.raises(ValueError, match="xtol"):
        T.refine_gaussian_patches(np.zeros((1, 7, 7), np.float32), xtol=1e-3)


def test_analyze_sequence_writes_files_and_refuses_to_plot(tmp_path, tracked):
    mov = tc.movie("odd")
    with pytest.raises(NotImplementedError, match="visualize_tracks"):
        T.analyze_microscopy_sequence(mov, visualize=True)
    prefix = os.path.join(tmp_path, "run")
    tracks, det, _ = T.analyze_microscopy_sequence(mov, min_track_length=5, output_prefix=prefix)
    import pandas as pd
    assert pd.read_csv(prefix + "_detections.csv").equals(det)
    with open(prefix + "_tracks.pkl", "rb") as fh:
        assert pickle.load(fh) == tracks == tracked["odd"][0]


def test_extract_particle_patches_unchanged(tracked):
    """The function that was here before keeps its behaviour: zero padding at the border, numpy in -> numpy out."""
    mov = tc.movie("odd")
    out = T.extract_particle_patches(mov, {0: [(0, 0, 0), (1, 50.5, 60.49)]}, patch_size=7)
    assert out[0].shape == (2, 7, 7) and (out[0][0, :3] == 0).all() and (out[0][0, :, :3] == 0).all()
    assert np.array_equal(out[0][1], mov[1, 47:54, 57:64])
