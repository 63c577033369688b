"""svgpu_reloc_solve_batch: every output of every candidate equals, byte for byte, the chain svgpu_pnp_ransac -> svgpu_pose_optimize ->
one-candidate svgpu_reloc_refine_batch with the host steps between them written in numpy (`chain` of tests/reloc_solve_problems.py) --
status, the poses as raw 64-bit patterns, every flag and count.  No tolerance, no exempted entry.  The yardstick of a problem is computed
once and shared.  The tests call the symbol itself: without it they fail."""
import ctypes as C

import numpy as np
import pytest

from tests import pnp_problems as PP
from tests import reloc_refine_problems as RP
from tests import reloc_solve_problems as SP

pytestmark = pytest.mark.gpu
REFINE_KEYS = ("tdesc", "t_xy", "t_octave", "t_angle", "t_xright", "scale_factors", "inv_level_sigma_sq", "log_scale_factor", "intrinsics", "pose_cw",
               "n_already_found", "frame_has_lm", "frame_lm_pos_w", "kf_off", "pos_w", "valid", "min_valid_dist", "max_valid_dist", "lm_desc", "angle_kf",
               "margin", "hamm_dist_thr", "min_num_valid_obs", "active", "check_orientation", "num_trials_robust", "num_trials", "num_each_iter",
               "reset_stop_flag_each_round", "grid_cols", "grid_rows")
SOLVE_KEYS = tuple(k for k in REFINE_KEYS if k not in ("pose_cw", "n_already_found", "frame_has_lm", "frame_lm_pos_w")) + (
    "t_bearings", "match_off", "m_keypt", "m_pos_w", "m_kf_entry", "samples", "min_num_inliers", "recompute", "gauss_newton_num_iter", "min_num_opt_valid_obs")


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


@pytest.fixture(scope="module")
def problems():
    return SP.classes()


def _solve(ctx, p, **over):
    from stella_vslam_amd import relocalizer
    assert hasattr(relocalizer.lib(), "svgpu_reloc_solve_batch")
    kw = {k: p[k] for k in SOLVE_KEYS}
    kw.update(over)
    return relocalizer.solve_batch(ctx, SP.camera(p), want_stats=True, **kw)


def device_backend(ctx):
    from stella_vslam_amd import relocalizer, solve

    def do_pnp(p, brg, pos, octv, samples):
        r = solve.pnp_ransac(ctx, brg, pos, octv, p["scale_factors"], samples, p["min_num_inliers"], bool(p["recompute"]), p["gauss_newton_num_iter"])
        return int(r["valid"][0]), r["pose_cw"][0].reshape(12), r["is_inlier"], int(r["best_iter"][0])

    def do_opt(p, pose, pos_w, uvr, w, hb):
        return RP.device_backend(ctx, SP.camera(p))[1](p, pose, pos_w, uvr, w, hb)

    def do_refine(one):
        return relocalizer.refine_pose_batch(ctx, SP.camera(one), **{k: one[k] for k in REFINE_KEYS})
    return do_pnp, do_opt, do_refine


_YARD = {}


def _chain(ctx, p, key, **over):
    if key not in _YARD:
        _YARD[key] = SP.chain(p, device_backend(ctx), **over)
    return _YARD[key]


def _check(ctx, p, key, **over):
    want, got = _chain(ctx, p, key, **over), _solve(ctx, p, **over)
    assert SP.same(got, want) == [], (key, got["status"], want["status"], got["opt_num_valid"], want["opt_num_valid"])
    return got


@pytest.mark.parametrize("name", tuple(SP.EXPECT))
def test_batch_equals_the_chain_of_single_calls(ctx, problems, name):
    got = _check(ctx, problems[name], name)
    assert got["status"].tolist() == SP.EXPECT[name]


@pytest.mark.parametrize("recompute", (0, 1))
def test_recompute_and_three_candidates(ctx, problems, recompute):
    p = dict(SP.sub(problems["each_status"], [5, 0, 3]), recompute=recompute)
    _check(ctx, p, ("three", recompute))


def _first_matches(p, c, n):
    """candidate c alone with the first n of its matches"""
    q = SP.sub(p, [c])
    for k in ("m_keypt", "m_pos_w", "m_kf_entry"):
        q[k] = np.ascontiguousarray(q[k][:n])
    q["match_off"] = np.array([0, n], np.int32)
    q["samples"] = PP.draw_samples(np.random.default_rng(50 + n), n, p["num_iter"])[None]
    return q


@pytest.mark.parametrize("n", (0, 3, SP.MIN_INLIERS - 1, SP.MIN_INLIERS))
def test_match_count_boundaries(ctx, problems, n):
    q = _first_matches(problems["accepted"], 0, n)
    got = _check(ctx, q, ("first", n))
    if n < SP.MIN_INLIERS:
        assert got["status"].tolist() == [SP.PNP_FAILED] and not got["pnp_valid"][0] and got["best_iter"][0] == -1 and not got["pose_out"].any()
    else:
        assert got["status"][0] in (SP.PNP_FAILED, SP.OPTIMIZE_FAILED)  # ten matches run; more than ten inliers there cannot be


def test_optimise_threshold_planted_from_the_measured_count(ctx, problems):
    p = SP.sub(problems["accepted"], [1])
    nv = int(_chain(ctx, p, "opt_base")["opt_num_valid"][0])
    assert nv >= 30
    at = _check(ctx, p, ("opt_at", nv), min_num_opt_valid_obs=nv)          # opt_num_valid == threshold: goes on
    above = _check(ctx, p, ("opt_above", nv), min_num_opt_valid_obs=nv + 1)  # == threshold - 1: stops, the pose goes on
    assert at["status"][0] == 0 and above["status"].tolist() == [SP.OPTIMIZE_FAILED]
    assert above["opt_num_valid"][0] == nv and above["pose_out"].tobytes() == above["opt_pose"].tobytes() == at["opt_pose"].tobytes()
    assert not above["num_found"].any() and (above["match_kf"] == -1).all()


def test_no_match_names_a_keyframe_entry(ctx, problems):
    p = SP.sub(problems["accepted"], [0, 2])
    p["m_kf_entry"] = np.full_like(p["m_kf_entry"], -1)
    _check(ctx, p, "no_entry_named")


def test_every_offered_entry_is_already_found(ctx, problems):
    p = SP.sub(problems["accepted"], [3])
    base = _chain(ctx, p, "found_base")
    held = (base["is_inlier"] != 0) & (base["opt_outlier"] == 0) & (p["m_kf_entry"] >= 0)
    valid = np.zeros_like(p["valid"])
    valid[p["m_kf_entry"][held]] = 1
    got = _check(ctx, dict(p, valid=valid), "all_found", min_num_valid_obs=int(base["opt_num_valid"][0]))
    assert held.sum() >= 20 and not got["num_found"].any()  # nothing left to project


def test_order_and_company_do_not_matter(ctx, problems):
    p = problems["accepted"]
    K = p["num_candidates"]
    full = _solve(ctx, p)
    rev = list(range(K))[::-1]
    got = _solve(ctx, SP.sub(p, rev))
    for k in SP.PER_CAND:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(full[k][rev]).tobytes(), k
    for k in SP.PER_MATCH:
        assert got[k].tobytes() == full[k][SP.match_rows(p, rev)].tobytes(), k
    for k in SP.PER_ENTRY:
        assert got[k].tobytes() == full[k][RP.rows_of(p, rev)].tobytes(), k
    for c in range(K):
        one = _solve(ctx, SP.sub(p, [c]))
        for k in SP.PER_CAND:
            assert np.ascontiguousarray(one[k]).tobytes() == np.ascontiguousarray(full[k][c:c + 1]).tobytes(), (c, k)
        for k in SP.PER_MATCH:
            assert one[k].tobytes() == full[k][SP.match_rows(p, [c])].tobytes(), (c, k)
        for k in SP.PER_ENTRY:
            assert one[k].tobytes() == full[k][RP.rows_of(p, [c])].tobytes(), (c, k)


def test_stats_do_not_depend_on_k_and_synchronise_no_more_than_the_refine_call(ctx, problems):
    from stella_vslam_amd import relocalizer
    p = problems["accepted"]
    s1, s5 = _solve(ctx, SP.sub(p, [0]))["stats"], _solve(ctx, p)["stats"]
    assert s1 == s5, (s1, s5)
    r = RP.sub(RP.classes()["all_accepted"], [0])
    ref = relocalizer.refine_pose_batch(ctx, SP.camera(r), want_stats=True, **{k: r[k] for k in REFINE_KEYS})["stats"]
    assert r["num_stages"] == p["num_stages"] and s5[2] <= ref[2], (s5, ref)


def _raw(ctx, p, **over):
    """the C call itself with every output pre-filled with a sentinel; returns (status code, outputs)"""
    from stella_vslam_amd._lib import lib, ptr
    a = dict(p)
    a.update(over)
    K, nt, S, N, M = p["num_candidates"], p["nt"], max(a["num_stages"], 1), int(p["kf_off"][-1]), int(p["match_off"][-1])
    outs = [np.full(K, 77, np.int32), np.full(K, 77, np.uint8), np.full((K, 12), 7.5), np.full(M, 77, np.uint8), np.full(K, 77, np.int32), np.full((K, 12), 7.5),
            np.full(M, 77, np.uint8), np.full(K, 77, np.int32), np.full((K, 12), 7.5), np.full(N, 77, np.int32), np.full(N, 77, np.int32),
            np.full(K * nt, 77, np.uint8), np.full(K * S, 77, np.int32), np.full(K * S, 77, np.int32), np.full(K, 77, np.int32)]
    cam = SP.camera(p)
    c = lambda k, t: None if a[k] is None else ptr(np.ascontiguousarray(a[k], t))
    rc = lib().svgpu_reloc_solve_batch(
        ctx.handle, C.byref(cam), c("tdesc", np.uint8), c("t_xy", np.float32), c("t_octave", np.int32), c("t_angle", np.float32), c("t_xright", np.float32),
        c("t_bearings", np.float64), nt, a["grid_cols"], a["grid_rows"], a["num_levels"], c("scale_factors", np.float32), c("inv_level_sigma_sq", np.float32),
        a["log_scale_factor"], c("intrinsics", np.float64), 2, 2, 10, 0, a["check_orientation"], K, c("active", np.uint8), c("match_off", np.int32),
        c("m_keypt", np.int32), c("m_pos_w", np.float64), c("m_kf_entry", np.int32), a["min_num_inliers"], a["num_iter"], c("samples", np.uint32), 0, 10,
        a["min_num_opt_valid_obs"], c("kf_off", np.int32), c("pos_w", np.float64), c("valid", np.uint8), c("min_valid_dist", np.float32),
        c("max_valid_dist", np.float32), c("lm_desc", np.uint8), c("angle_kf", np.float32), a["num_stages"], c("margin", np.float32), c("hamm_dist_thr", np.int32),
        a["min_num_valid_obs"], *[ptr(o) for o in outs], None)
    return rc, outs


def test_invalid_arguments_launch_nothing_and_touch_nothing(ctx, problems):
    p = problems["accepted"]
    off, mo = p["kf_off"], p["match_off"]

    def changed(key, index, value):
        a = p[key].copy()
        a.reshape(-1)[index] = value
        return {key: a}
    m1 = int(mo[1])
    named = np.flatnonzero(p["m_kf_entry"][:m1] >= 0)
    cases = dict(
        null_bearings=dict(t_bearings=None), null_matches=dict(m_keypt=None), null_positions=dict(m_pos_w=None), null_entries=dict(m_kf_entry=None),
        null_match_off=dict(match_off=None), null_kf_off=dict(kf_off=None), null_samples=dict(samples=None), null_desc=dict(tdesc=None), null_margin=dict(margin=None),
        match_off_first=changed("match_off", 0, 1), match_off_non_monotone=changed("match_off", 2, int(mo[1]) - 1),
        kf_off_first=changed("kf_off", 0, 1), kf_off_non_monotone=changed("kf_off", 2, int(off[1]) - 1),
        keypt_negative=changed("m_keypt", 0, -1), keypt_beyond=changed("m_keypt", m1 - 1, p["nt"]), keypt_equal=changed("m_keypt", 1, int(p["m_keypt"][0])),
        keypt_descending=changed("m_keypt", 5, int(p["m_keypt"][3])),
        entry_low=changed("m_kf_entry", 0, -2), entry_beyond=changed("m_kf_entry", 0, int(off[1] - off[0])),
        entry_repeated=changed("m_kf_entry", int(named[0]), int(p["m_kf_entry"][named[1]])),
        sample_beyond=changed("samples", 2, m1), sample_repeated=changed("samples", 5, int(p["samples"].reshape(-1)[4])),
        octave_high=changed("t_octave", 5, p["num_levels"]), octave_negative=changed("t_octave", 0, -1), no_stage=dict(num_stages=0), five_stages=dict(num_stages=5))
    for name, over in cases.items():
        rc, outs = _raw(ctx, p, **over)
        assert rc == 1, (name, rc)  # SVGPU_ERR_INVALID
        for o in outs:
            assert (o == (7.5 if o.dtype == np.float64 else 77)).all(), name
    rc, outs = _raw(ctx, p)  # the same call, unchanged, runs
    assert rc == 0 and (outs[0] == 0).all()


def test_no_candidate_succeeds_with_null_pointers(ctx):
    from stella_vslam_amd._lib import lib
    assert lib().svgpu_reloc_solve_batch(ctx.handle, *([None] * 7), 0, 0, 0, 0, None, None, 0.0, None, 0, 0, 0, 0, 0, 0, *([None] * 5), 0, 0, None, 0, 0, 0,
                                         *([None] * 7), 0, None, None, 0, *([None] * 16)) == 0
    assert lib().svgpu_reloc_solve_batch(ctx.handle, *([None] * 7), -3, -1, -1, 99, None, None, -1.0, None, -1, -1, -1, 0, 0, 0, *([None] * 5), -1, -1, None, 0, -1,
                                         -5, *([None] * 7), 9, None, None, 0, *([None] * 16)) == 0  # whatever else is passed
