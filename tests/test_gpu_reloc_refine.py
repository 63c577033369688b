"""svgpu_reloc_refine_batch: every output of the batch equals, element for element and bit for bit, the same chain composed of the existing
single calls svgpu_match_frame_and_keyframe_projection and svgpu_pose_optimize one candidate at a time (compose_single_calls of
tests/reloc_refine_problems.py) -- status, poses as raw 64-bit patterns, match_kf, match_stage, outlier, the counts and lm_iterations.
The yardstick of a class is computed once, shared by the tests and never changed."""
import ctypes as C
import types

import numpy as np
import pytest

from oracle import oracle as O
from tests import reloc_refine_problems as RP

pytestmark = pytest.mark.gpu
CLASSES = ("all_accepted", "each_status", "inactive", "degenerate", "one_stage", "four_stages", "stereo", "fisheye", "equirect", "no_orientation",
           "twins", "many_tiny")
KEYS = ("tdesc", "t_xy", "t_octave", "t_angle", "t_xright", "scale_factors", "inv_level_sigma_sq", "log_scale_factor", "intrinsics", "pose_cw",
        "n_already_found", "frame_has_lm", "frame_lm_pos_w", "kf_off", "pos_w", "valid", "min_valid_dist", "max_valid_dist", "lm_desc", "angle_kf",
        "margin", "hamm_dist_thr", "min_num_valid_obs", "active", "check_orientation", "num_trials_robust", "num_trials", "num_each_iter",
        "reset_stop_flag_each_round", "grid_cols", "grid_rows")


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


@pytest.fixture(scope="module")
def problems():
    return RP.classes()


def _cam(problem):
    c = problem["cam"]  # (the oracle's Camera is laid out as svgpu_camera and fills the image bounds as the reference's constructors do)
    return O.make_camera(c["model"], c["cols"], c["rows"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"], c["focal_x_baseline"])


def _batch(ctx, problem, **over):
    from stella_vslam_amd import relocalizer
    kw = {k: problem[k] for k in KEYS}
    kw.update(over)
    return relocalizer.refine_pose_batch(ctx, _cam(problem), want_stats=True, **kw)


_YARD = {}


def _yardstick(ctx, problem, **over):
    key = (problem["name"], tuple(sorted(over.items())))
    if key not in _YARD:
        p = dict(problem, **over)
        _YARD[key] = RP.compose_single_calls(p, RP.device_backend(ctx, _cam(p)))
    return _YARD[key]


@pytest.mark.parametrize("name", CLASSES)
def test_batch_equals_the_composed_single_calls(ctx, problems, name):
    p = problems[name]
    want, got = _yardstick(ctx, p), _batch(ctx, p)
    assert RP.same(got, want) == [], (name, got["status"], want["status"], got["num_found"], want["num_found"])
    if name in RP.EXPECT:
        assert got["status"].tolist() == RP.EXPECT[name]


@pytest.mark.parametrize("name", ("each_status", "degenerate", "stereo"))
def test_order_and_company_do_not_matter(ctx, problems, name):
    p = problems[name]
    K = p["num_candidates"]
    full = _batch(ctx, p)
    assert RP.same(_batch(ctx, p), full) == []  # the same call twice
    rev = list(range(K))[::-1]
    got = _batch(ctx, RP.sub(p, rev))
    rows = RP.rows_of(p, rev)
    for k in ("status", "pose_out", "outlier", "num_found", "num_valid", "lm_iterations"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(full[k][rev]).tobytes(), (name, k)
    assert np.array_equal(got["match_kf"], full["match_kf"][rows]) and np.array_equal(got["match_stage"], full["match_stage"][rows])
    for c in range(K):  # each candidate alone equals its row of the batch
        one = _batch(ctx, RP.sub(p, [c]))
        r = RP.rows_of(p, [c])
        for k in ("status", "pose_out", "outlier", "num_found", "num_valid", "lm_iterations"):
            assert np.ascontiguousarray(one[k]).tobytes() == np.ascontiguousarray(full[k][c:c + 1]).tobytes(), (name, c, k)
        assert np.array_equal(one["match_kf"], full["match_kf"][r]) and np.array_equal(one["match_stage"], full["match_stage"][r])


def _predicted(base, n_already, S, m):
    """the status the chain of count tests gives candidate 0 at threshold m: the counts of the stages it reaches do not depend on m"""
    count = n_already
    for s in range(S):
        if count + int(base["num_found"][0, s]) < m:
            return 1 + s
        count = int(base["num_valid"][0, s])
    return 1 + S if count < m else 0


@pytest.mark.parametrize("name,keep", [("all_accepted", [2, 0]), ("four_stages", [1, 0])])
def test_decision_boundaries_planted_from_measured_counts(ctx, problems, name, keep):
    """for one candidate with matches in several stages, at every stage: min_num_valid_obs = count + num_found[s] passes that test, one more
    fails it; likewise the final num_valid.  One threshold serves every test of the chain, so for a later cut the FIRST test is taken out
    of the way through n_already_found, a number that enters nothing else; the status asserted is the one the measured counts predict, and
    at c + 1 it is 1 + s unless a test between the first and s already fails at that threshold."""
    p = RP.sub(problems[name], keep)
    p["name"] = name + "_boundary"
    base = _yardstick(ctx, p)
    S = p["num_stages"]
    assert base["status"][0] == 0
    count = int(p["n_already_found"][0])
    cuts = []
    for s in range(S):
        cuts.append((count + int(base["num_found"][0, s]), 1 + s))
        count = int(base["num_valid"][0, s])
    cuts.append((count, 1 + S))
    seen = set()
    for c, failed in cuts:
        big = 10000 if failed > 1 else int(p["n_already_found"][0])
        q = dict(p, name=f"{name}_boundary{failed}", n_already_found=np.array([big, p["n_already_found"][1]], np.int32))
        for m in (c, c + 1):
            want = _yardstick(ctx, q, min_num_valid_obs=m)
            got = _batch(ctx, q, min_num_valid_obs=m)
            assert RP.same(got, want) == [], (c, m)
            st = int(got["status"][0])
            assert st == _predicted(base, big, S, m), (name, c, m, st)
            if m == c:
                assert st == 0 or st > failed, (c, m, st)   # the planted test passes
            else:
                assert 0 < st <= failed, (c, m, st)         # and fails one above (or an earlier test of the chain does)
                if failed == 1:
                    assert st == 1
            seen.add(st)
    # (which later statuses a threshold can reach is decided by the counts: a test behind the first fails alone only where the valid count
    #  fell or the stage found something; the exact status is asserted above either way)
    assert {0, 1} <= seen and len(seen) >= 3, (name, seen)


def test_launches_and_synchronisations_do_not_depend_on_k(ctx, problems):
    p = problems["all_accepted"]
    eight = RP.sub(p, [0, 1, 2, 3, 0, 1, 2, 3])
    s1, s8 = _batch(ctx, RP.sub(p, [0]))["stats"], _batch(ctx, eight)["stats"]
    assert s1[0] == s8[0] and s1[2] == s8[2], (s1, s8)
    assert s1[2] == p["num_stages"] + 1  # one total per stage, one at the end


def test_lists_that_outgrow_their_capacity_restart_the_call(ctx, problems):
    """a first-stage window of 200 px x scale lists about a third of the frame per entry, more than the 64 entries per keyframe entry the lists
    are first sized for: the call starts again with longer lists (more than stages + 1 synchronisations) and still equals the yardstick"""
    p = dict(problems["all_accepted"], name="wide_window", margin=np.array([200.0, 3.0], np.float32))
    want, got = _yardstick(ctx, p), _batch(ctx, p)
    assert RP.same(got, want) == []
    assert got["stats"][2] > p["num_stages"] + 1, got["stats"]
    assert (got["status"] == 0).all()


def _raw(ctx, p, **over):
    """the C call itself with every output pre-filled with a sentinel; returns (status code, outputs)"""
    from stella_vslam_amd._lib import lib, ptr
    a = {k: p[k] for k in p}
    a.update(over)
    K, nt, S = a["num_candidates"], a["nt"], a["num_stages"]
    N = int(p["kf_off"][-1])
    Ko, nto = (p["num_candidates"], p["nt"]) if a.pop("small_outputs", False) else (K, nt)  # (a call refused on its sizes writes nothing)
    outs = [np.full(Ko, 77, np.int32), np.full((Ko, 12), 7.5), np.full(N, 77, np.int32), np.full(N, 77, np.int32), np.full(Ko * nto, 77, np.uint8),
            np.full(Ko * max(S, 1), 77, np.int32), np.full(Ko * max(S, 1), 77, np.int32), np.full(Ko, 77, np.int32)]
    cam = _cam(p)
    c = lambda k, t: None if a[k] is None else np.ascontiguousarray(a[k], t)
    keep = [c("tdesc", np.uint8), c("t_xy", np.float32), c("t_octave", np.int32), c("t_angle", np.float32), c("t_xright", np.float32), c("scale_factors", np.float32),
            c("inv_level_sigma_sq", np.float32), c("intrinsics", np.float64), c("active", np.uint8), c("pose_cw", np.float64), c("n_already_found", np.int32),
            c("frame_has_lm", np.uint8), c("frame_lm_pos_w", np.float64), c("kf_off", np.int32), c("pos_w", np.float64), c("valid", np.uint8),
            c("min_valid_dist", np.float32), c("max_valid_dist", np.float32), c("lm_desc", np.uint8), c("angle_kf", np.float32), c("margin", np.float32),
            c("hamm_dist_thr", np.int32)]
    k = [ptr(x) for x in keep]
    rc = lib().svgpu_reloc_refine_batch(ctx.handle, C.byref(cam), k[0], k[1], k[2], k[3], k[4], nt, a["grid_cols"], a["grid_rows"], a["num_levels"], k[5], k[6],
                                        a["log_scale_factor"], k[7], 2, 2, 10, 0, a["check_orientation"], K, k[8], k[9], k[10], k[11], k[12], k[13], k[14], k[15],
                                        k[16], k[17], k[18], k[19], S, k[20], k[21], a["min_num_valid_obs"], *[ptr(o) for o in outs], None)
    return rc, outs


def test_invalid_arguments_launch_nothing_and_touch_nothing(ctx, problems):
    p = problems["all_accepted"]
    off = p["kf_off"]
    bad_oct = p["t_octave"].copy()
    bad_oct[5] = p["num_levels"]
    neg_oct = p["t_octave"].copy()
    neg_oct[0] = -1
    cases = dict(first_offset=dict(kf_off=off + np.int32(1) * (np.arange(len(off)) == 0)), non_monotone=dict(kf_off=np.array([0, off[2], off[1], off[3], off[4]], np.int32)),
                 octave_high=dict(t_octave=bad_oct), octave_negative=dict(t_octave=neg_oct), no_stage=dict(num_stages=0), five_stages=dict(num_stages=5),
                 null_pose=dict(pose_cw=None), null_offsets=dict(kf_off=None), null_desc=dict(tdesc=None), null_entries=dict(pos_w=None),
                 null_margin=dict(margin=None), null_state=dict(frame_has_lm=None),
                 too_many_keypoints=dict(nt=1 << 22, small_outputs=True),
                 # totals that do not fit int32 (600 x 2^20 keypoint slots x 4): refused on the sizes and the offsets alone, before any
                 # per-keypoint array is read
                 totals_beyond_int32=dict(num_candidates=600, nt=1 << 20, kf_off=np.zeros(601, np.int32), small_outputs=True))
    for name, over in cases.items():
        rc, outs = _raw(ctx, p, **over)
        assert rc == 1, (name, rc)  # SVGPU_ERR_INVALID
        for o in outs:
            assert (o == (7.5 if o.dtype == np.float64 else 77)).all(), name


def test_no_candidate_succeeds_with_null_pointers(ctx):
    from stella_vslam_amd._lib import lib
    assert lib().svgpu_reloc_refine_batch(ctx.handle, *([None] * 6), 0, 0, 0, 0, None, None, 0.0, None, 0, 0, 0, 0, 0, 0, *([None] * 12), 0, None, None, 0,
                                          *([None] * 9)) == 0
    assert lib().svgpu_reloc_refine_batch(ctx.handle, *([None] * 6), -3, -1, -1, 99, None, None, -1.0, None, -1, -1, -1, 0, 0, 0, *([None] * 12), 9, None, None, 0,
                                          *([None] * 9)) == 0  # whatever else is passed


def test_single_projection_call_is_what_the_oracle_says(ctx, problems):
    """the single entry point on these problems, against the CPU oracle's restatement of the matcher (its body is shared with no one: the batch
    reuses the device functions it is made of)"""
    from stella_vslam_amd import match
    for name in ("all_accepted", "stereo", "fisheye", "equirect", "no_orientation"):
        p = problems[name]
        cam = _cam(p)
        lo, hi = int(p["kf_off"][0]), int(p["kf_off"][1])
        T = p["pose_cw"][0].reshape(3, 4)
        for margin, thr in zip(p["margin"], p["hamm_dist_thr"]):
            kw = dict(rot_cw=np.ascontiguousarray(T[:, :3]), trans_cw=np.ascontiguousarray(T[:, 3]), pos_w=p["pos_w"][lo:hi], valid=p["valid"][lo:hi],
                      min_valid_dist=p["min_valid_dist"][lo:hi], max_valid_dist=p["max_valid_dist"][lo:hi], lm_desc=p["lm_desc"][lo:hi], angle_kf=p["angle_kf"][lo:hi],
                      scale_factors=p["scale_factors"], log_scale_factor=p["log_scale_factor"], margin=float(margin), hamm_dist_thr=int(thr), tdesc=p["tdesc"],
                      t_xy=p["t_xy"], t_octave=p["t_octave"], t_angle=p["t_angle"], occupied=p["frame_has_lm"][0])
            got, num = match.projection_flat(0.9, bool(p["check_orientation"]), ctx).match_frame_and_keyframe(types.SimpleNamespace(c_=cam), **kw)
            ref, rnum = O.match_frame_and_keyframe_projection(bool(p["check_orientation"]), cam, **kw)
            assert np.array_equal(got, ref) and num == rnum, (name, margin)
