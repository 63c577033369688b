"""The PnP yardstick (tests/pnp_problems.py) on its own, on the CPU: the restatement of solve::pnp_solver recovers the planted pose on every
problem class, and the conditions tests/test_gpu_pnp.py relies on hold for the restatement alone -- at least 90 % of the over-determined
sets have a unique pose (the four smallest singular values of M^T M pairwise separated by a relative 1e-6), at least 90 % of the planted
RANSAC problems select the planted inliers under three bases of the null space, and the selection rule is the reference's."""
import numpy as np
import pytest

from tests import pnp_problems as T


def _rot_err(R, R0):
    return float(np.abs(np.asarray(R) - R0).max())


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("n", [6, 63, 64, 65, 300])
def test_noise_free_sets_recover_the_planted_pose(kind, n):
    p = T.planted(7, n, kind)
    for dtype in (np.float64, np.longdouble):
        R, t, err, _ = T.compute_pose(p["bearings"], p["pos_w"], dtype=dtype)
        scale = max(1.0, np.abs(p["t"]).max())
        assert _rot_err(R, p["R"]) < 1e-9 and np.abs(t - p["t"]).max() < 1e-9 * scale, (kind, n, dtype, _rot_err(R, p["R"]))
        assert abs(np.linalg.det(R) - 1.0) < 1e-9 and err < 1e-12


def test_equirectangular_bearings_exercise_the_sign_flip():
    p = T.planted(3, 64, "equirect")
    assert (p["bearings"][:, 2] < 0).all()
    R, t, _, _ = T.compute_pose(p["bearings"], p["pos_w"])
    assert ((p["pos_w"] @ R.T + t)[:, 2] < 0).all()


def test_coplanar_landmarks_exercise_the_pseudo_inverse_rule():
    p = T.planted(3, 64, "coplanar")
    pw0 = p["pos_w"] - p["pos_w"].mean(0)
    s = np.linalg.svd(pw0.T @ pw0, compute_uv=False)
    assert np.sqrt(s[2] / 64) <= 1e-6 < np.sqrt(s[1] / 64)   # D(2) of CC falls under the rule, D(1) does not
    _, _, _, sv = T.compute_pose(p["bearings"], p["pos_w"])
    assert T.null_gap(sv) < 1e-6                               # ... and the pose has no unique null-space basis: excluded from the parity class


@pytest.mark.parametrize("noise", [0.0, 1e-3])
def test_at_least_nine_in_ten_overdetermined_sets_have_a_unique_pose(noise):
    sets = T.pose_sets(noise)
    assert {len(p["pos_w"]) for p in sets} == set(T.OVERDETERMINED)
    gaps = [T.null_gap(T.compute_pose(p["bearings"], p["pos_w"])[3]) for p in sets]
    assert sum(g >= 1e-6 for g in gaps) >= 0.9 * len(sets), sorted(gaps)[:5]


def test_far_landmarks_are_far():
    p = T.planted(1, 65, "far")
    assert 5e2 < np.linalg.norm(p["pos_w"], axis=1).min() and np.linalg.norm(p["pos_w"], axis=1).max() < 5e3


def test_max_cos_errors_follow_the_octave():
    sf = T.orb_scale_factors()
    m = T.max_cos_errors(np.arange(8), sf)
    assert m.dtype == np.float32 and (np.diff(m) < 0).all()
    assert abs(float(m[0]) - np.cos(np.pi / 180.0)) < 1e-3   # util::cos is a degree-4 polynomial: about 6e-4 off


def test_selection_rule_is_strict_and_keeps_the_first_of_equal_costs():
    assert T.select([20, 20, 20], [3.0, 2.0, 2.0], 10) == 1
    assert T.select([10, 11], [1.0, 5.0], 10) == 1            # num_inliers > min_num_inliers, strict
    assert T.select([20, 20], [np.nan, np.nan], 10) == -1     # a NaN cost never wins
    assert T.select([20, 20, 20], [np.nan, 4.0, np.nan], 10) == 1
    assert T.select([5, 5], [1.0, 1.0], 10) == -1


def test_small_problems_are_invalid():
    sf = T.orb_scale_factors()
    for n, min_inl in ((3, 0), (9, 10)):
        p = T.planted(2, n, "pinhole")
        r = T.find_via_ransac(p["bearings"], p["pos_w"], p["octaves"], sf, np.zeros((5, 4), np.uint32), min_inl)
        assert not r["valid"] and r["best_iter"] == -1 and not r["is_inlier"].any()


def test_no_hypothesis_passes_min_num_inliers():
    p = T.planted(4, 80, "pinhole", outliers=0.2)
    smp = T.draw_samples(np.random.default_rng(1), 80, 6)
    r = T.find_via_ransac(p["bearings"], p["pos_w"], p["octaves"], p["scale_factors"], smp, 80)
    assert not r["valid"]


def test_batches_cover_the_sizes_and_the_degenerate_problems():
    sizes = [len(p["pos_w"]) for p in T.ransac_batch(17)]
    assert set(T.MATCH_COUNTS) <= set(sizes) and 0 in sizes and 3 in sizes and max(sizes) == 300
    assert [len(T.ransac_batch(k)) for k in (1, 3, 17)] == [1, 3, 17]


def test_planted_ransac_problems_select_the_planted_inliers_under_three_bases():
    kept, probs = T.outcome_problems()
    assert len(kept) >= 0.9 * len(probs), (len(kept), len(probs))


def test_drop_in_sampling_follows_the_references_random_array():
    """solve::hip::pnp_solver with use_fixed_seed draws the sample tables that util::create_random_engine(true) and
    util::create_random_array(4, 0U, n - 1, engine) gave when the reference's own util/random_array.cc was built and run
    (tests/golden/pnp_random_array.json: n = 80, 5, 300, 30 iterations each, a fresh engine per n)."""
    import json
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parent.parent
    exe = root / "stella_vslam_amd" / "host" / "test_pnp_solver"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    got = json.loads(subprocess.run([str(exe), "--draws"], capture_output=True, text=True, check=True).stdout)
    ref = json.loads((root / "tests" / "golden" / "pnp_random_array.json").read_text())["draws"]
    assert len(got) == len(ref) == 3
    for g, r in zip(got, ref):
        assert np.asarray(g).reshape(-1, 4).tolist() == r["samples"], r["num_matches"]
