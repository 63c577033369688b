"""GPU parity of the projection family on its gate boundaries: every planted class of tests/reproj_problems.py through the device entry
points (reproject_landmarks and the five projection-family matchers of svgpu_match2.hip), against the CPU oracle on the same problem.
Every boundary is planted where the deciding arithmetic is exact, so nothing is filtered: match lists and counts are identical, and for
reproject_landmarks visible / pred_level / reproj / x_right are bit-identical (equirectangular positions, which go through asin / atan2,
keep the 1e-11 of tests/test_gpu_frame.py).  The planted expectation itself is asserted too, so a failure names the gate."""
import numpy as np
import pytest

from tests import reproj_problems as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backends():
    from stella_vslam_amd import camera, feature, match
    ctx = feature.Context()
    made = {}

    def cam(spec):
        key = tuple(sorted(spec.items()))
        if key not in made:
            setup = "Stereo" if spec["fxb"] else "Monocular"
            a = ("planted", setup, "Gray", spec["cols"], spec["rows"], 30.0, spec["fx"], spec["fy"], spec["cx"], spec["cy"])
            if spec["model"] == "perspective":
                made[key] = camera.perspective(*a, 0, 0, 0, 0, 0, focal_x_baseline=spec["fxb"], ctx=ctx)
            elif spec["model"] == "fisheye":
                made[key] = camera.fisheye(*a, 0, 0, 0, 0, focal_x_baseline=spec["fxb"], ctx=ctx)
            elif spec["model"] == "radial_division":
                made[key] = camera.radial_division(*a, 0.0, focal_x_baseline=spec["fxb"], ctx=ctx)
            else:
                made[key] = camera.equirectangular("planted", "Gray", spec["cols"], spec["rows"], 30.0, ctx=ctx)
            if spec["model"] != "equirectangular":   # the bounds the classes plant on
                assert made[key].img_bounds_.as_tuple() == (0.0, float(spec["cols"]), 0.0, float(spec["rows"]))
        return made[key]

    def reproject(c, R, t, pw, nv, mn, mx, thr, levels, lsf, valid):
        return c.reproject_landmarks(R, t, pw, nv, mn, mx, thr, levels, lsf, skip=(valid == 0).astype(np.uint8))
    flat = lambda check: match.projection_flat(0.9, check, ctx)
    dev = dict(cam=cam, reproject_landmarks=reproject,
               current_last=lambda check, c, **kw: flat(check).match_current_and_last_frames(c, **kw),
               frame_keyframe=lambda check, c, **kw: flat(check).match_frame_and_keyframe(c, **kw),
               sim3=lambda c, **kw: flat(False).match_by_Sim3_transform(c, **kw),
               mutually=lambda c1, c2, **kw: flat(False).match_keyframes_mutually(c1, c2, **kw),
               fuse=lambda c, **kw: match.fuse(0.6, ctx).detect_duplication(c, **kw))
    return dev, P.oracle_backend()


def _differences(p, got, ref):
    """where the device leaves the oracle (everything compared, nothing excused), then where it leaves the planted expectation"""
    bad = []
    if p.ep == "reproject_landmarks":
        names = ("visible", "reproj", "x_right", "pred_level")
        for name, g, r in zip(names, got, ref):
            if name == "reproj" and p.cam["model"] == "equirectangular":   # asin / atan2 of two math libraries (tests/test_gpu_frame.py's bound)
                same = g.shape == r.shape and np.abs(g - r).max(initial=0.0) < 1e-11
            else:
                same = g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
            if not same:
                bad.append((name, np.flatnonzero((np.asarray(g) != np.asarray(r)).reshape(len(g), -1).any(1)).tolist()))
        if not np.array_equal(got[0] != 0, np.array(p.vis, bool)):
            bad.append(("planted", np.flatnonzero((got[0] != 0) != np.array(p.vis, bool)).tolist()))
        return bad
    for k, (g, r, e) in enumerate(zip(got, ref, p.expected())):
        if not np.array_equal(g, r):
            bad.append((f"result {k} against the oracle", np.flatnonzero(np.asarray(g) != np.asarray(r)).tolist() if np.ndim(g) else (g, r)))
        if not np.array_equal(g, e):
            bad.append((f"result {k} against the plant", np.flatnonzero(np.asarray(g) != np.asarray(e)).tolist() if np.ndim(g) else (g, e)))
    return bad


def _class_test(cls):
    @pytest.mark.parametrize("ep,model", P.cells(cls))
    def test(backends, ep, model):
        dev, orc = backends
        probs = [p for p in P.problems_of(cls) if (p.ep, p.cam["model"]) == (ep, model)]
        assert probs
        bad = []
        for p in probs:
            d = _differences(p, p.run(dev), p.run(orc))
            if d:
                bad.append((p.cls, p.ep, p.name, d))
        assert not bad, bad   # (class, entry point, problem, [(which output, landmark indices)])
    test.__name__ = test.__qualname__ = f"test_{cls}"
    test.__doc__ = P.CLASSES[cls].__doc__
    return test


test_image_bounds = _class_test("image_bounds")
test_distance_float = _class_test("distance_float")
test_distance_double = _class_test("distance_double")
test_no_distance_test = _class_test("no_distance_test")
test_ray_cosine = _class_test("ray_cosine")
test_half_dot = _class_test("half_dot")
test_no_normal_test = _class_test("no_normal_test")
test_sim3_center = _class_test("sim3_center")
test_scale_level = _class_test("scale_level")
test_level_window = _class_test("level_window")
test_margin = _class_test("margin")
test_window_cells = _class_test("window_cells")
test_stereo_gate = _class_test("stereo_gate")
test_chi_gate = _class_test("chi_gate")
test_offered = _class_test("offered")
