"""The planted classes of tests/reproj_problems.py on the CPU: the oracle returns every planted expectation (so each triple straddles its
boundary and the private-keypoint construction isolates one gate), no plant sits near a scale-level tie except the exact ones, every
class is non-empty for every entry point the mode table assigns to it, and -- where oracle/_ref holds the reference's own compiled
matchers and cameras -- the reference's matchers return the same lists and its cameras the planted bounds.  frame::can_observe of the
reference is not run on the plants: its export (tests/test_ref_local_camera.py) lets the reference derive each landmark's normal and
valid-distance range from an observation, so a planted range or normal cannot be handed to it."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import reproj_problems as P

_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libsvref.so")


@pytest.fixture(scope="module")
def backend():
    return P.oracle_backend()


def check(p, res):
    """a result of Problem.run against the planted expectation; returns a description of the first difference or None"""
    if p.ep == "reproject_landmarks":
        vis = res[0]
        if not np.array_equal(vis != 0, np.array(p.vis, bool)):
            return (p.cls, p.ep, p.name, "visible", np.flatnonzero((vis != 0) != np.array(p.vis, bool)).tolist())
        lvl = np.array([l["level"] if v else -1 for l, v in zip(p.lm, p.vis)], np.int32).reshape(-1)   # the planted level of what is visible
        if p.cam["model"] != "equirectangular" and not np.array_equal(res[3], lvl):
            return (p.cls, p.ep, p.name, "pred_level", np.flatnonzero(res[3] != lvl).tolist())
        return None
    exp = p.expected()
    for k, (g, e) in enumerate(zip(res, exp)):
        if not np.array_equal(g, e):
            return (p.cls, p.ep, p.name, k, np.flatnonzero(np.asarray(g) != np.asarray(e)).tolist() if np.ndim(g) else (g, e))
    return None


@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_oracle_returns_every_planted_expectation(backend, cls):
    bad = [b for b in (check(p, p.run(backend)) for p in P.problems_of(cls)) if b]
    assert not bad, bad


@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_class_covers_its_entry_points_and_stays_small(cls):
    probs = P.problems_of(cls)
    assert {p.ep for p in probs} == set(P.TABLE[cls])
    for ep in P.TABLE[cls]:
        assert sum(len(p.lm) for p in probs if p.ep == ep) > 0, (cls, ep)
    for p in probs:
        assert len(p.lm) <= 48 and len(p.kp) <= 48 and p.cls == cls
        assert len(p.vis) == len(p.lm) == len(p.expect)
    if cls == "image_bounds":
        assert {p.cam["model"] for p in probs} == set(P.PINHOLE) | {"equirectangular"}
        for m in P.PINHOLE:
            assert {p.ep for p in probs if p.cam["model"] == m} == set(P.ENTRY_POINTS)
    # both outcomes are planted in every class that has a boundary
    if cls not in ("no_distance_test", "no_normal_test"):
        assert any(p.vis.count(True) for p in probs) and any(p.vis.count(False) for p in probs)


@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_no_level_ties(cls):
    """log(ratio) / log_scale_factor stays 1e-5 away from an integer (the margin of test_gpu_match2._no_level_ties) for every plant of every
    class, except the scale_level plants that sit on an exact tie (ratio == 1) or within one float of it"""
    for p in P.problems_of(cls):
        t = p.level_ties()
        assert not t or min(t) > 1e-5, (cls, p.ep, p.name, min(t))
        assert not p.exact_level or cls == "scale_level"


def test_descriptors_isolate():
    d = np.array([P.hadamard_desc(i) for i in range(255)])
    bits = np.unpackbits(d, axis=1).astype(np.int32)
    ham = (bits[:, None, :] != bits[None, :, :]).sum(2)
    assert (ham[~np.eye(255, dtype=bool)] == 128).all()


# --------------------------------------------------------------------------------------------- the reference's own compiled matchers
@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(_SO):
        pytest.skip("oracle/_ref/libsvref.so absent: it is built from the reference checkout by `make -C oracle/ref_local` (build container only)")
    return C.CDLL(_SO)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _c(a, t):
    return None if a is None else np.ascontiguousarray(a, t)


def _replay(out, n_targets, occupied=None):
    holder = np.full(n_targets, -1, np.int32)
    if occupied is not None:
        holder[np.asarray(occupied) != 0] = -2
    for q, t in enumerate(out):
        if t >= 0:
            holder[t] = q
    return holder


def _ref_backend(ref):
    """the exports tests/test_ref_local_match.py uses, behind the oracle wrappers' signatures.  They build their scale tables from
    (1.2, num_levels) themselves -- the tables of reproj_problems -- and the frame-writing ones return the holder of every keypoint."""
    sf = C.c_float(1.2), P.LEVELS
    f64 = lambda a: np.ascontiguousarray(a, np.float64)

    def current_last(check, cam, rot_cw, trans_cw, rot_lw, trans_lw, pos_w, valid, lm_desc, octave_last, angle_last, scale_factors, margin, tdesc, t_xy,
                     t_octave, t_angle, occupied=None, t_xright=None, lm_has_observation=None, is_monocular=True, true_baseline=0.0):
        a = [f64(rot_cw), f64(trans_cw), f64(rot_lw), f64(trans_lw), f64(pos_w), _c(valid, np.uint8), _c(lm_desc, np.uint8), _c(octave_last, np.int32),
             _c(angle_last, np.float32), _c(lm_has_observation, np.uint8), _c(tdesc, np.uint8), _c(t_xy, np.float32), _c(t_octave, np.int32),
             _c(t_angle, np.float32), _c(occupied, np.uint8), _c(t_xright, np.float32)]
        nt = len(a[10])
        holder = np.full(nt, -9, np.int32)
        num = ref.svref_match_current_and_last_frames(C.byref(cam), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), int(is_monocular), C.c_float(true_baseline), len(a[4]),
                                                      _p(a[4]), _p(a[5]), _p(a[6]), _p(a[7]), _p(a[8]), _p(a[9]), *sf, C.c_float(margin), _p(a[10]), _p(a[11]),
                                                      _p(a[12]), _p(a[13]), nt, _p(a[14]), _p(a[15]), 64, 48, int(check), _p(holder))
        return ("holder", holder, occupied), num

    def frame_keyframe(check, cam, rot_cw, trans_cw, pos_w, valid, min_valid_dist, max_valid_dist, lm_desc, angle_kf, scale_factors, log_scale_factor, margin,
                       hamm_dist_thr, tdesc, t_xy, t_octave, t_angle, occupied=None):
        a = [f64(rot_cw), f64(trans_cw), f64(pos_w), _c(valid, np.uint8), _c(min_valid_dist, np.float32), _c(max_valid_dist, np.float32), _c(lm_desc, np.uint8),
             _c(angle_kf, np.float32), _c(tdesc, np.uint8), _c(t_xy, np.float32), _c(t_octave, np.int32), _c(t_angle, np.float32), _c(occupied, np.uint8)]
        nt = len(a[8])
        holder = np.full(nt, -9, np.int32)
        num = ref.svref_match_frame_and_keyframe_projection(C.byref(cam), _p(a[0]), _p(a[1]), len(a[2]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), _p(a[6]), _p(a[7]),
                                                            *sf, C.c_float(margin), int(hamm_dist_thr), _p(a[8]), _p(a[9]), _p(a[10]), _p(a[11]), nt, _p(a[12]),
                                                            64, 48, int(check), _p(holder))
        return ("holder", holder, occupied), num

    def sim3(cam, sim3_cw, pos_w, valid, min_valid_dist, max_valid_dist, mean_normal, lm_desc, scale_factors, log_scale_factor, margin, tdesc, t_xy, t_octave,
             occupied=None):
        a = [f64(sim3_cw), f64(pos_w), _c(valid, np.uint8), _c(min_valid_dist, np.float32), _c(max_valid_dist, np.float32), f64(mean_normal), _c(lm_desc, np.uint8),
             _c(tdesc, np.uint8), _c(t_xy, np.float32), _c(t_octave, np.int32), _c(occupied, np.uint8)]
        nt = len(a[7])
        holder = np.full(nt, -9, np.int32)
        num = ref.svref_match_by_sim3_transform(C.byref(cam), _p(a[0]), len(a[1]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), _p(a[6]), *sf, C.c_float(margin),
                                                _p(a[7]), _p(a[8]), _p(a[9]), nt, _p(a[10]), 64, 48, _p(holder))
        return ("holder", holder, occupied), num

    def mutually(cam1, cam2, rot_1w, trans_1w, rot_2w, trans_2w, s_12, rot_12, trans_12, kf1, kf2, scale_factors, log_scale_factor, margin):
        side = lambda k: [f64(k["pos_w"]), _c(k["valid"], np.uint8), _c(k["min_valid_dist"], np.float32), _c(k["max_valid_dist"], np.float32),
                          _c(k["lm_desc"], np.uint8), _c(k["desc"], np.uint8), _c(k["xy"], np.float32), _c(k["octave"], np.int32)]
        s1, s2 = side(kf1), side(kf2)
        a = [f64(rot_1w), f64(trans_1w), f64(rot_2w), f64(trans_2w), f64(rot_12), f64(trans_12)]
        out = np.full(len(s1[0]), -9, np.int32)
        num = ref.svref_match_keyframes_mutually(C.byref(cam2), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), C.c_float(s_12), _p(a[4]), _p(a[5]), len(s1[0]),
                                                 *[_p(x) for x in s1], len(s2[0]), *[_p(x) for x in s2], *sf, C.c_float(margin), 64, 48, _p(out))
        return ("mutual", out), num

    def fuse(cam, rot_cw, trans_cw, pos_w, valid, min_valid_dist, max_valid_dist, mean_normal, lm_desc, scale_factors, inv_level_sigma_sq, log_scale_factor,
             margin, tdesc, t_xy, t_octave, t_xright=None, do_reprojection_matching=False):
        a = [f64(rot_cw), f64(trans_cw), f64(pos_w), _c(valid, np.uint8), _c(min_valid_dist, np.float32), _c(max_valid_dist, np.float32), f64(mean_normal),
             _c(lm_desc, np.uint8), _c(tdesc, np.uint8), _c(t_xy, np.float32), _c(t_octave, np.int32), _c(t_xright, np.float32)]
        out = np.full(len(a[2]), -9, np.int32)
        num = ref.svref_fuse_detect_duplication(C.byref(cam), _p(a[0]), _p(a[1]), len(a[2]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), _p(a[6]), _p(a[7]), *sf,
                                                C.c_float(margin), int(do_reprojection_matching), _p(a[8]), _p(a[9]), _p(a[10]), _p(a[11]), len(a[8]), 64, 48, _p(out))
        return out, num
    return dict(cam=P.oracle_cam, current_last=current_last, frame_keyframe=frame_keyframe, sim3=sim3, mutually=mutually, fuse=fuse)


def _ref_runs(p):
    """the reference's matcher exports take this problem: a matcher with landmarks and keypoints, one camera for both keyframes"""
    if p.ep not in P.MATCHERS or not p.lm or (p.ep == "mutually" and "cam1" in p.opt):
        return False
    return p.ep == "mutually" or bool(p.kp)


_MATCHER_CLASSES = [c for c in P.CLASSES if set(P.TABLE[c]) & set(P.MATCHERS)]


def test_classes_held_against_the_reference_matchers():
    """every class the mode table gives to a matcher reaches the compiled reference, through every matcher of the class"""
    assert set(P.CLASSES) - set(_MATCHER_CLASSES) == {"distance_float", "ray_cosine"}     # reproject_landmarks only
    for cls in _MATCHER_CLASSES:
        assert {p.ep for p in P.problems_of(cls) if _ref_runs(p)} == set(P.TABLE[cls]) & set(P.MATCHERS), cls


@pytest.mark.parametrize("cls", _MATCHER_CLASSES)
def test_reference_agrees_with_the_oracle(ref, backend, cls):
    """every planted problem of the five matchers through match/projection.cc and match/fuse.cc themselves, and -- the oracle has been
    held to the plant above -- through them against the planted expectation"""
    rb = _ref_backend(ref)
    bad, compared = [], 0
    for p in P.problems_of(cls):
        if not _ref_runs(p):
            continue
        o = p.run(backend)
        r, rnum = p.run(rb)
        if p.ep == "mutually":
            ok = np.array_equal(r[1], o[2]) and rnum == o[3]
        elif p.ep == "fuse":
            ok = np.array_equal(r, o[0]) and rnum == o[1]
        else:
            ok = np.array_equal(r[1], _replay(o[0], len(p.kp), r[2])) and rnum == o[1]
        compared += len(p.lm)
        if not ok:
            bad.append((cls, p.ep, p.name))
    assert compared > 0, cls
    assert not bad, bad


# The matcher exports reach the image through the oracle's reproject_to_image (their camera is a stand-in around it), so the bounds of
# image_bounds are held against the reference's own camera classes here, compiled into a library of their own.
_SO_CAM = os.path.join(os.path.dirname(_SO), "libsvref_cam.so")


@pytest.fixture(scope="module")
def ref_cam():
    if not os.path.exists(_SO_CAM):
        pytest.skip("oracle/_ref/libsvref_cam.so absent: it is built from the reference checkout by `make -C oracle/ref_local` (build container only)")
    return C.CDLL(_SO_CAM)


@pytest.mark.parametrize("model", P.PINHOLE + ("equirectangular",))
def test_reference_cameras_return_the_planted_bounds(ref_cam, model):
    """camera::*::reproject_to_image itself on every position of image_bounds: strict bounds for perspective and fisheye, inclusive ones
    for radial division, the depth test at and around Z == 0.  In these plants nothing but the camera decides, so its return value is
    the planted visibility; the oracle's camera returns the same, with the same image point bit for bit where it is inside."""
    probs = [p for p in P.problems_of("image_bounds") if p.ep == "reproject_landmarks" and p.cam["model"] == model]
    assert len(probs) == 1
    p = probs[0]
    s, n = p.cam, len(p.lm)
    pw = np.ascontiguousarray([l["pos"] for l in p.lm], np.float64)
    R, t, d = np.eye(3), np.zeros(3), np.zeros(5)
    ok, rp, xr, bok, bear = np.zeros(n, np.uint8), np.zeros((n, 2)), np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros((n, 3))
    cd = C.c_double
    ref_cam.svref_camera_reproject(P._MODEL[model], 0, s["cols"], s["rows"], cd(s.get("fx", 0)), cd(s.get("fy", 0)), cd(s.get("cx", 0)), cd(s.get("cy", 0)),
                                   _p(d), cd(0.0), _p(R), _p(t), n, _p(pw), _p(ok), _p(rp), _p(xr), _p(bok), _p(bear))
    assert n > 0 and np.array_equal(ok != 0, np.array(p.vis, bool)), np.flatnonzero((ok != 0) != np.array(p.vis, bool)).tolist()
    if model != "equirectangular":   # (its positions go through asin / atan2)
        assert 0 < ok.sum() < n
        cam, L = P.oracle_cam(s), P.O.lib()
        for i in range(n):
            r2, x1 = np.zeros(2), C.c_float(0)
            assert bool(L.orc_reproject_to_image(C.byref(cam), _p(R), _p(t), _p(pw[i]), _p(r2), C.byref(x1))) == bool(ok[i]), i
            if ok[i]:
                assert r2.tobytes() == rp[i].tobytes() and np.float32(x1.value) == xr[i], i
