"""CPU checks of the two-view triangulation yardstick (tests/triangulation_problems.py): every problem class drives the path it is named
for on the restatement alone, the share of matches that sit within 1e-9 of a threshold stays under the cap the GPU test relies on, a
closed-form case comes back, and the new entry points refuse NULL arguments without a device."""
import ctypes as C

import numpy as np
import pytest

from tests import triangulation_problems as T

MARGIN, CAP = 1e-9, 1e-3


@pytest.fixture(scope="module")
def classes():
    return T.problem_classes()


@pytest.fixture(scope="module")
def results(classes):
    return {name: [T.restate_problem(p) for p in ps] for name, ps in classes.items()}


def _all(results, name, key):
    return np.concatenate([r[key] for r in results[name]])


def test_every_status_code_occurs(results):
    seen = set()
    for name in results:
        seen |= set(_all(results, name, "status").tolist())
    assert {T.ACCEPTED, T.NO_MODE, T.DEPTH, T.REPROJECTION, T.SCALE, T.SKIPPED} <= seen


@pytest.mark.parametrize("name", ["perspective_mono", "fisheye", "radial_division", "equirectangular", "absent_arrays", "size_20000"])
def test_monocular_classes_triangulate_linearly(results, classes, name):
    br, st = _all(results, name, "branch"), _all(results, name, "status")
    assert set(br.tolist()) <= {T.LINEAR, T.NONE}
    assert (st == T.ACCEPTED).mean() > 0.5 and (st == T.NO_MODE).any()
    for p in classes[name]:
        assert p["view1"]["cam"]["model"] == p["view2"]["cam"]["model"]


def test_accepted_matches_recover_the_planted_points(results, classes):
    p, r = classes["perspective_mono"][0], results["perspective_mono"][0]
    acc = r["status"] == T.ACCEPTED
    err = np.linalg.norm(r["pos_w"][acc] - p["planted"][acc], axis=1) / np.linalg.norm(p["planted"][acc], axis=1)
    assert np.median(err) < 0.05


def test_equirectangular_skips_the_depth_test(results, classes):
    p, r = classes["equirectangular"][0], results["equirectangular"][0]
    acc = r["status"] == T.ACCEPTED
    pc = T.project(p["view1"]["cam"], p["view1"]["pose_cw"], r["pos_w"])[3]
    assert (pc[acc, 2] < 0).sum() > 100  # accepted points behind the "front" of the panorama
    assert not (r["status"] == T.DEPTH).any()


@pytest.mark.parametrize("name,branches", [("stereo_stereo", {T.LINEAR, T.STEREO_1, T.STEREO_2}), ("stereo_mono", {T.LINEAR, T.STEREO_1}),
                                           ("mono_stereo", {T.LINEAR, T.STEREO_2})])
def test_stereo_classes_reach_their_branches(results, name, branches):
    br, st = _all(results, name, "branch"), _all(results, name, "status")
    for b in branches:
        assert ((br == b) & (st == T.ACCEPTED)).sum() >= 50, b
    assert set(br.tolist()) <= branches | {T.NONE}


def test_parallax_class_straddles_the_threshold(results):
    for r in results["parallax_straddle"]:
        share = (r["branch"] == T.LINEAR).mean()
        assert 0.1 < share < 0.9


def test_points_behind_one_camera_fail_the_depth_test(results):
    st = _all(results, "behind_one_camera", "status")
    assert (st == T.DEPTH).sum() > 100


def test_gross_outliers_meet_both_chi_square_gates(results, classes):
    for p, r in zip(classes["gross_outliers"], results["gross_outliers"]):
        assert (r["status"] == T.REPROJECTION).sum() > 300 and (r["status"] == T.ACCEPTED).sum() > 300
    assert classes["gross_outliers"][1]["view1"]["xright"] is not None  # the 3-dof gate


def test_octave_pairs_straddle_the_ratio_factor(results):
    st = _all(results, "octave_straddle", "status")
    assert (st == T.SCALE).sum() > 100 and (st == T.ACCEPTED).sum() > 100


def test_identical_poses_have_no_parallax(results):
    assert (_all(results, "identical_poses", "status") == T.NO_MODE).all()


def test_matched_2_in_1_form_has_unmatched_entries(results, classes):
    for p, r in zip(classes["matched_2_in_1"], results["matched_2_in_1"]):
        assert p["idx2"] is None and len(p["idx1"]) == len(p["view1"]["octave"])
        assert ((p["idx1"] < 0) == (r["status"] == T.SKIPPED)).all() and (p["idx1"] < 0).sum() >= 300


def test_sizes(classes):
    assert [len(p["idx1"]) for p in classes["sizes"]] == [0, 1, 63, 64, 65]
    assert len(classes["size_20000"][0]["idx1"]) == 20000


def test_absent_arrays(classes):
    for v in ("view1", "view2"):
        assert classes["absent_arrays"][0][v]["xright"] is None and classes["absent_arrays"][0][v]["depth"] is None
    assert classes["mono_stereo"][0]["view1"]["xright"] is None and classes["mono_stereo"][0]["view2"]["xright"] is not None


def test_exact_threshold_cases_decide_as_designed(results, classes):
    for p, r in zip(classes["exact_thresholds"], results["exact_thresholds"]):
        assert p["exact"] and (r["status"] == p["expect"]).all(), p["name"]
    eq = classes["exact_thresholds"][0]
    assert np.array_equal(eq["view1"]["depth"], eq["view2"]["depth"])


def test_share_of_matches_on_a_threshold_is_under_the_cap(results, classes):
    """The GPU test excuses a status difference only where the margin is below 1e-9, and at most 0.1 % of a class: the yardstick itself must
    stay inside that cap on every class without exemption-free inputs."""
    for name, ps in classes.items():
        if all(p["exact"] for p in ps):
            continue
        m = _all(results, name, "margin")
        if len(m):
            share = (m < MARGIN).mean()
            print(f"{name}: {len(m)} matches, share with margin < 1e-9 = {share:.2e}, < 1e-6 = {(m < 1e-6).mean():.2e}")
            assert share <= CAP, name


def test_closed_form_planted_points_come_back():
    c = T.closed_form()
    for null in (T.null_svd, T.null_jacobi, lambda A: T.null_jacobi(A, np.float64, 12)):
        pos = null(T.build_A(c["b1"], c["b2"], c["P1"], c["P2"]))
        err = np.linalg.norm(pos - c["planted"], axis=1) / np.linalg.norm(c["planted"], axis=1)
        assert err.max() < 1e-9, err.max()


def test_numpy_and_extended_precision_null_vectors_agree(classes):
    """The calibration the GPU test uses: deviation of the fp64 LAPACK null vector from the long double Jacobi on one class."""
    p = classes["size_20000"][0]
    a, b = T.restate_problem(p), T.restate_problem(p, "longdouble")
    acc = (a["status"] == T.ACCEPTED) & (b["status"] == T.ACCEPTED)
    dev = np.linalg.norm(a["pos_w"][acc] - b["pos_w"][acc], axis=1) / np.linalg.norm(b["pos_w"][acc], axis=1)
    print(f"numpy fp64 vs long double: max {dev.max():.2e}, median {np.median(dev):.2e}")
    assert dev.max() < 1e-9


def test_new_entry_points_refuse_null_arguments():
    from stella_vslam_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert L.svgpu_triangulate_two_views(*([None] * 3), C.c_double(0), *([None] * 5), 0, *([None] * 2), C.c_double(0), *([None] * 5), 0, None, None, 0,
                                         C.c_float(1.2), C.c_float(1.2), C.c_float(1.0), None, None, 0, None, None, None) == 1  # SVGPU_ERR_INVALID
    assert L.svgpu_triangulate_two_views_batch(None, None, None, 0, None, None, None, 0, C.c_float(1.0), None, None, None, None, None) == 1
