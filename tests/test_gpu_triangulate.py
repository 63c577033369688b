"""svgpu_triangulate_two_views / _batch on the device against the CPU restatement of module::two_view_triangulator::triangulate
(tests/triangulation_problems.py).

Status: equal to the restatement for every match; a match whose smallest relative distance from any threshold is below 1e-9 may differ, at
most 0.1 % of a class, and never in the classes built from exactly representable inputs.  Position of accepted matches: against the long
double null vector, within 16 x the deviation numpy's own fp64 SVD shows on the same class (floored at 1e-12); stereo-branch positions
within 1e-14.  Measured on an MI355X (largest figures over all classes): numpy deviation 4.7e-13, tolerance 7.5e-12, device deviation 4.9e-13
(equirectangular; 2.2e-14 on the pinhole classes) -- DESIGN.md section 9."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from tests import triangulation_problems as T

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
MARGIN, CAP = 1e-9, 1e-3


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


def _view(v):
    from stella_vslam_amd.camera import svgpu_camera
    cam, c = v["cam"], svgpu_camera()
    c.model, c.cols, c.rows, c.fx, c.fy, c.cx, c.cy = cam["model"], cam["cols"], cam["rows"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    c.focal_x_baseline = cam["focal_x_baseline"]
    c.min_x, c.max_x, c.min_y, c.max_y = cam["bounds"]
    return dict(v, cam=c)


def _run(ctx, p):
    from stella_vslam_amd import match
    return match.triangulate_two_views(ctx, _view(p["view1"]), _view(p["view2"]), p["tables"]["scale_factors"], p["tables"]["level_sigma_sq"], p["idx1"],
                                       p["idx2"], p["deg_thr"])


def _rel_dev(a, b):
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


@pytest.mark.parametrize("name", sorted(T.problem_classes().keys()))
def test_status_and_position_against_the_restatement(ctx, name):
    problems = T.problem_classes()[name]
    total = excused = 0
    for p in problems:
        ref, ext = T.restate_problem(p), T.restate_problem(p, "longdouble")
        pos, st, num = _run(ctx, p)
        assert len(st) == len(ref["status"]) and num == int((st == T.ACCEPTED).sum())
        diff = st != ref["status"]
        if p["exact"]:
            assert not diff.any(), (p["name"], np.flatnonzero(diff)[:10], st[diff][:10], ref["status"][diff][:10])
        else:
            assert (ref["margin"][diff] < MARGIN).all(), (p["name"], np.flatnonzero(diff)[:10], st[diff][:10], ref["status"][diff][:10], ref["margin"][diff][:10])
        total, excused = total + len(st), excused + int(diff.sum())
        acc = (st == T.ACCEPTED) & (ref["status"] == T.ACCEPTED) & (ext["status"] == T.ACCEPTED)
        lin, ste = acc & (ref["branch"] == T.LINEAR), acc & (ref["branch"] != T.LINEAR)
        if lin.any():
            numpy_dev = _rel_dev(ref["pos_w"][lin], ext["pos_w"][lin]).max()
            tol = max(16.0 * numpy_dev, 1e-12)
            dev = _rel_dev(pos[lin], ext["pos_w"][lin])
            print(f"{p['name']}: {int(lin.sum())} linear, numpy deviation {numpy_dev:.3e}, tolerance {tol:.3e}, device deviation max {dev.max():.3e} median {np.median(dev):.3e}")
            assert dev.max() <= tol, (p["name"], dev.max(), tol)
        if ste.any():
            dev = _rel_dev(pos[ste], ref["pos_w"][ste])
            print(f"{p['name']}: {int(ste.sum())} stereo-branch, device deviation max {dev.max():.3e}")
            assert dev.max() <= 1e-14, (p["name"], dev.max())
    assert excused <= CAP * total, (name, excused, total)


def _neighbour_set(k):
    """k neighbours of one current keyframe, with different cameras and one neighbour without matches (k >= 3)."""
    nbs, idx1, idx2, off, sides, base = [], [], [], [0], [], 0
    specs = [dict(model2=T.PERSPECTIVE), dict(model2=T.FISHEYE, stereo=(False, True), centre2=(0.08, 0.0, 0.25), depth_noise=0.02, dmax=12.0),
             dict(model2=T.RADIAL_DIVISION, centre2=(-0.3, 0.05, 0.1)), dict(model2=T.EQUIRECTANGULAR, centre2=(0.2, -0.2, 0.0))]
    for j in range(k):
        n = 0 if (k >= 3 and j == 1) else 250 + 37 * j
        # one seed: the same pose and camera of keyframe 1 in every pair; its keypoints are the concatenation of the pairs' side-1 keypoints
        p = T.make_pair(100, n, name=f"nb{j}", **specs[j % len(specs)])
        sides.append(p["view1"])
        assert np.array_equal(p["view1"]["pose_cw"], sides[0]["pose_cw"]) and p["view1"]["cam"] == sides[0]["cam"]
        nbs.append(p["view2"])
        idx1.append(p["idx1"] + base)
        idx2.append(p["idx2"])
        base += len(p["view1"]["octave"])
        off.append(off[-1] + n)
    v1 = dict(sides[0])
    for key in ("xy", "octave", "bearings", "xright", "depth"):
        v1[key] = np.concatenate([v[key] for v in sides])
    return v1, nbs, np.concatenate(idx1).astype(np.int32), np.concatenate(idx2).astype(np.int32), np.asarray(off, np.int32), p["tables"]


@pytest.mark.parametrize("k", [1, 3, 10])
def test_batch_equals_single_calls_bit_for_bit(ctx, k):
    from stella_vslam_amd import match
    v1, nbs, idx1, idx2, off, tb = _neighbour_set(k)
    g1, gn = _view(v1), [_view(v) for v in nbs]
    pos, st, num = match.triangulate_two_views_batch(ctx, g1, gn, off, tb["scale_factors"], tb["level_sigma_sq"], idx1, idx2)
    assert (st == T.ACCEPTED).sum() > 0
    for j in range(k):
        a, b = off[j], off[j + 1]
        ps, ss, ns = match.triangulate_two_views(ctx, g1, gn[j], tb["scale_factors"], tb["level_sigma_sq"], idx1[a:b], idx2[a:b])
        assert np.array_equal(ss, st[a:b]) and ns == num[j], j
        assert ps.tobytes() == pos[a:b].tobytes(), j
        ref = T.restate(v1, nbs[j], tb, idx1[a:b], idx2[a:b])
        diff = ss != ref["status"]
        assert (ref["margin"][diff] < MARGIN).all(), j


def test_matcher_output_feeds_the_triangulator(ctx):
    """svgpu_match_for_triangulation's matched_2_in_1 goes straight in and equals the pair-list form."""
    from tests import match_problems as MP
    from stella_vslam_amd import match
    sc = MP.scene(seed=7)
    gcam = MP.make_cams(sc, "svgpu")
    kw = MP.triangulation(sc, lambda R, t, c: match.reproject_to_bearing(gcam, R, t, c))
    m21, num = match.match_for_triangulation(ctx, 0.8, True, **kw)
    assert num > 20
    a, b = sc["views"][0], sc["views"][1]
    fx, fy, cx, cy, fxb = sc["K"]
    cam = T.camera(T.PERSPECTIVE, cols=sc["width"], rows=sc["height"], fx=fx, fy=fy, cx=cx, cy=cy, true_baseline=fxb / fx)
    tb = dict(T.orb_tables(), scale_factors=np.asarray(sc["tables"]["scale_factors"], np.float32))
    tb["level_sigma_sq"] = (tb["scale_factors"] * tb["scale_factors"]).astype(np.float32)
    views = []
    for v, brg in ((a, kw["bearings1"]), (b, kw["bearings2"])):
        pose = np.concatenate([np.asarray(v["rot_cw"], np.float64), np.asarray(v["trans_cw"], np.float64)[:, None]], 1)
        views.append(dict(cam=cam, pose_cw=pose, true_baseline=cam["true_baseline"], xy=np.asarray(v["xy"], np.float32), octave=np.asarray(v["octave"], np.int32),
                          bearings=np.asarray(brg, np.float64), xright=None, depth=None, scale_factor=tb["scale_factor"]))
    g = [_view(v) for v in views]
    pos_m, st_m, n_m = match.triangulate_two_views(ctx, g[0], g[1], tb["scale_factors"], tb["level_sigma_sq"], m21, None)
    has = m21 >= 0
    pos_p, st_p, n_p = match.triangulate_two_views(ctx, g[0], g[1], tb["scale_factors"], tb["level_sigma_sq"], np.flatnonzero(has), m21[has])
    assert (st_m[~has] == T.SKIPPED).all() and np.array_equal(st_m[has], st_p) and n_m == n_p
    assert pos_m[has].tobytes() == pos_p.tobytes()
    ref = T.restate(views[0], views[1], tb, np.flatnonzero(has), m21[has])
    diff = st_p != ref["status"]
    assert (ref["margin"][diff] < MARGIN).all()


def test_equirectangular_stereo_keypoint_is_refused(ctx):
    from stella_vslam_amd._lib import SvgpuError
    p = T.make_pair(50, 10, T.EQUIRECTANGULAR, name="equirect_stereo")
    p["view1"]["xright"] = np.full(len(p["view1"]["octave"]), 5.0, np.float32)
    with pytest.raises(SvgpuError) as e:
        _run(ctx, p)
    assert e.value.status == 1


def test_out_of_range_index_is_refused(ctx):
    from stella_vslam_amd._lib import SvgpuError
    p = T.make_pair(51, 10, name="bad_index")
    p["idx2"] = p["idx2"].copy()
    p["idx2"][3] = len(p["view2"]["octave"])
    with pytest.raises(SvgpuError) as e:
        _run(ctx, p)
    assert e.value.status == 1


def test_drop_in_class_agrees_with_itself_and_the_c_abi():
    """host/drop_in/two_view_triangulator_hip: single-match and batch forms on stand-in keyframes, mono and stereo, against the C ABI."""
    exe = ROOT / "stella_vslam_amd" / "host" / "test_two_view_triangulator"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "two_view_triangulator ok" in out.stdout
