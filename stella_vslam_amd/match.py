"""Python mirror of stella_vslam::match::* over the C ABI (flat-array form).

The reference matchers take frame / keyframe / landmark objects (match/robust.h, match/projection.h).
Here a "frame observation" is the flat part of data::frame_observation (data/frame_observation.h:12-38):
`descriptors` (N x 32 uint8) and `keypts` (structured array with at least `angle`, `octave`).
Constructor arguments and thresholds are the reference's (match/base.h:15-17,81-91).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, ptr as _p
from .feature import Context

HAMMING_DIST_THR_LOW = 50
HAMMING_DIST_THR_HIGH = 100
MAX_HAMMING_DIST = 256

MATCH_BEST_ONLY = 0
MATCH_RATIO_SAME_OCTAVE = 1
MATCH_RATIO = 2          # bow_tree::match_frame_and_keyframe / match_keyframes
MATCH_TRIANGULATION = 3  # bow_tree / robust ::match_for_triangulation
MATCH_AREA = 4           # area::match_in_consistent_area


def _c(a, t):
    return None if a is None else np.ascontiguousarray(a, t)


def compute_descriptor_distance_32(ctx: Context, desc_1: np.ndarray, desc_2: np.ndarray) -> np.ndarray:
    """match/base.h:20-41 for n row pairs."""
    a = np.ascontiguousarray(desc_1, np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(desc_2, np.uint8).reshape(-1, 32)
    out = np.zeros(len(a), np.uint32)
    ctx.check(lib().svgpu_hamming_distance(ctx.handle, _p(a), _p(b), len(a), _p(out)), "svgpu_hamming_distance")
    return out


def hamming_matrix(ctx: Context, desc1: np.ndarray, desc2: np.ndarray) -> np.ndarray:
    d1, d2 = _c(desc1, np.uint8), _c(desc2, np.uint8)
    out = np.zeros((len(d2), len(d1)), np.uint16)
    ctx.check(lib().svgpu_hamming_matrix(ctx.handle, _p(d1), len(d1), _p(d2), len(d2), _p(out)), "svgpu_hamming_matrix")
    return out


class base:
    def __init__(self, lowe_ratio: float, check_orientation: bool, ctx: Context | None = None):
        self.lowe_ratio_ = float(lowe_ratio)
        self.check_orientation_ = bool(check_orientation)
        self.ctx = ctx or Context()


class robust(base):
    """match/robust.h.  brute_force_match (match/robust.cc:232-328): returns the (idx_1, idx_2) pairs sorted by idx_1."""

    def brute_force_match(self, desc_1, angle_1, desc_2, angle_2, lm_valid_2=None):
        d1, d2 = _c(desc_1, np.uint8), _c(desc_2, np.uint8)
        a1, a2 = _c(angle_1, np.float32), _c(angle_2, np.float32)
        v2 = _c(lm_valid_2, np.uint8)
        out = np.full(len(d1), -1, np.int32)
        num = C.c_int(0)
        self.ctx.check(lib().svgpu_match_bruteforce(self.ctx.handle, _p(d1), _p(a1), len(d1), _p(d2), _p(a2), _p(v2), len(d2),
                                                    self.lowe_ratio_, int(self.check_orientation_), _p(out),
                                                    C.byref(num)), "svgpu_match_bruteforce")
        idx1 = np.flatnonzero(out >= 0)
        assert len(idx1) == num.value
        return [(int(i), int(out[i])) for i in idx1], out


class projection(base):
    """match/projection.h on flattened inputs: the caller supplies, per query (landmark / last-frame keypoint),
    the candidate keypoint indices that get_keypoints_in_cell returned (data/common.cc:127-190), as CSR."""

    def match_candidates(self, qdesc, tdesc, cand_off, cand_idx, mode, thr, cand_skip=None, t_octave=None, q_valid=None, occupied=None,
                         q_angle=None, t_angle=None, q_xright=None, t_xright=None, q_xr_tol=None):
        qd, td = _c(qdesc, np.uint8), _c(tdesc, np.uint8)
        off, idx = _c(cand_off, np.int32), _c(cand_idx, np.int32)
        toct, qv, occ = _c(t_octave, np.int32), _c(q_valid, np.uint8), _c(occupied, np.uint8)
        skip = _c(cand_skip, np.uint8)
        qa, ta = _c(q_angle, np.float32), _c(t_angle, np.float32)
        qx, tx, qt = _c(q_xright, np.float32), _c(t_xright, np.float32), _c(q_xr_tol, np.float32)
        out = np.full(len(qd), -1, np.int32)
        num = C.c_int(0)
        self.ctx.check(lib().svgpu_match_candidates(self.ctx.handle, _p(qd), len(qd), _p(td), _p(toct), len(td), _p(off), _p(idx),
                                                    _p(skip), _p(qv), _p(occ), _p(qa), _p(ta), int(self.check_orientation_), _p(qx),
                                                    _p(tx), _p(qt), thr, self.lowe_ratio_, mode, _p(out),
                                                    C.byref(num)), "svgpu_match_candidates")
        return out, num.value


    def match_in_cells(self, qdesc, q_xy, q_margin, tdesc, t_xy, t_octave, bounds, mode, thr, q_min_level=None, q_max_level=None,
                       q_valid=None, occupied=None, q_angle=None, t_angle=None, q_xright=None, t_xright=None, q_xr_tol=None,
                       grid_cols=64, grid_rows=48, q_blocks=None):
        """Same matcher, candidate lists built on the device: query q scans frm.get_keypoints_in_cell(q_xy[q], q_margin[q],
        q_min_level[q], q_max_level[q]) (data/common.cc:127-190) over the grid of data::assign_keypoints_to_grid."""
        qd, td = _c(qdesc, np.uint8), _c(tdesc, np.uint8)
        qxy, txy, qm = _c(q_xy, np.float32), _c(t_xy, np.float32), _c(q_margin, np.float32)
        toct, qlo, qhi = _c(t_octave, np.int32), _c(q_min_level, np.int32), _c(q_max_level, np.int32)
        qv, occ = _c(q_valid, np.uint8), _c(occupied, np.uint8)
        qa, ta = _c(q_angle, np.float32), _c(t_angle, np.float32)
        qx, tx, qt = _c(q_xright, np.float32), _c(t_xright, np.float32), _c(q_xr_tol, np.float32)
        out = np.full(len(qd), -1, np.int32)
        num = C.c_int(0)
        qb = _c(q_blocks, np.uint8)  # 0 = an accepted query does not close its keypoint (its landmark has no observation, projection.cc:52-55)
        if qb is not None:
            self.ctx.check(lib().svgpu_match_set_query_blocks(self.ctx.handle, _p(qb)), "svgpu_match_set_query_blocks")
        self.ctx.check(lib().svgpu_match_in_cells(self.ctx.handle, _p(qd), len(qd), _p(qxy), _p(qm), _p(qlo), _p(qhi), _p(qv), _p(qa), _p(qx),
                                                  _p(qt), _p(td), _p(txy), _p(toct), len(td), _p(occ), _p(ta), _p(tx),
                                                  bounds[0], bounds[1], bounds[2], bounds[3],
                                                  grid_cols, grid_rows, int(self.check_orientation_ and qa is not None and ta is not None), thr,
                                                  self.lowe_ratio_, mode, _p(out), C.byref(num)), "svgpu_match_in_cells")
        return out, num.value


    def match_frame_and_landmarks(self, camera, rot_cw, trans_cw, pos_w, mean_normal, min_valid_dist, max_valid_dist, lm_desc,
                                  frm_obs, scale_factors, log_scale_factor, margin=5.0, skip=None, occupied=None, ray_cos_thr=0.5,
                                  trans_wc=None):
        """tracking_module::search_local_landmarks' observability loop (tracking_module.cc:554-594 -> data/frame.cc:59-85)
        followed by projection::match_frame_and_landmarks (match/projection.cc:13-93) as ONE device pass: the landmarks come in
        as flat arrays (position, mean viewing direction, valid distance range, representative descriptor), `skip` marks the
        ones the caller's object graph excludes, `occupied` the keypoints that already hold an observed landmark.
        Returns (match_lm, num_matches, visible, reproj, x_right, pred_scale_level); match_lm[i] = keypoint index given to
        frm.add_landmark(lm_i, idx) or -1."""
        R = np.ascontiguousarray(rot_cw, np.float64).reshape(3, 3)
        t = np.ascontiguousarray(trans_cw, np.float64).reshape(3)
        twc = np.ascontiguousarray(-R.T @ t if trans_wc is None else trans_wc, np.float64)
        pw = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
        nv = np.ascontiguousarray(mean_normal, np.float64).reshape(-1, 3)
        mn, mx = _c(min_valid_dist, np.float32), _c(max_valid_dist, np.float32)
        qd = _c(lm_desc, np.uint8)
        sk, occ = _c(skip, np.uint8), _c(occupied, np.uint8)
        sf = _c(scale_factors, np.float32)
        td = _c(frm_obs.descriptors_, np.uint8)
        txy = np.ascontiguousarray(np.stack([frm_obs.undist_keypts_["x"], frm_obs.undist_keypts_["y"]], 1), np.float32)
        toct = _c(frm_obs.undist_keypts_["octave"], np.int32)
        tx = _c(frm_obs.stereo_x_right_, np.float32)
        n = len(pw)
        out = np.full(n, -1, np.int32)
        num = C.c_int(0)
        vis, rp, xr, lv = np.zeros(n, np.uint8), np.zeros((n, 2), np.float64), np.zeros(n, np.float32), np.zeros(n, np.int32)
        self.ctx.check(lib().svgpu_match_frame_and_landmarks(
            self.ctx.handle, C.byref(camera.c_), _p(R), _p(t), _p(twc), n, _p(pw), _p(nv), _p(mn), _p(mx), _p(sk), _p(qd),
            ray_cos_thr, len(sf), _p(sf), log_scale_factor, margin, _p(td), _p(txy), _p(toct), len(td),
            _p(occ), _p(tx), frm_obs.num_grid_cols_, frm_obs.num_grid_rows_, HAMMING_DIST_THR_HIGH, self.lowe_ratio_,
            _p(out), C.byref(num), _p(vis), _p(rp), _p(xr), _p(lv)), "svgpu_match_frame_and_landmarks")
        return out, num.value, vis, rp, xr, lv


class area(base):
    """match/area.h (the monocular initialiser's matcher).  match_in_consistent_area (match/area.cc:8-98) on flattened inputs:
    level-0 keypoints of frame 1 are the queries, the candidate list of query idx_1 is
    frm_2.get_keypoints_in_cell(prev_matched_pts[idx_1], margin, 0, 0) (empty for keypoints of higher levels), as CSR.
    Returns matched_indices_2_in_frm_1 and the number of matches; the caller then refreshes prev_matched_pts (:91-95)."""

    def match_in_consistent_area(self, desc_1, angle_1, desc_2, angle_2, cand_off, cand_idx):
        out, num = projection.match_candidates(self, desc_1, desc_2, cand_off, cand_idx, MATCH_AREA, 50, q_angle=angle_1, t_angle=angle_2)
        return out, num


class stereo:
    """match/stereo.h: stereo(left_pyramid, right_pyramid, keypts_left, keypts_right, descs_left, descs_right, scale_factors,
    inv_scale_factors, focal_x_baseline, true_baseline).compute() -> (stereo_x_right, depths).  The two pyramids are taken
    from the extractors that produced the keypoints (their last extract call), as system.cc:443-447 does."""

    def __init__(self, extractor_left, extractor_right, keypts_left, keypts_right, descs_left, descs_right,
                 focal_x_baseline: float, true_baseline: float):
        self.el, self.er = extractor_left, extractor_right
        self.kl, self.kr = np.ascontiguousarray(keypts_left), np.ascontiguousarray(keypts_right)
        self.dl, self.dr = _c(descs_left, np.uint8), _c(descs_right, np.uint8)
        self.focal_x_baseline_, self.true_baseline_ = float(focal_x_baseline), float(true_baseline)

    def compute(self):
        n = len(self.kl)
        xr, dp = np.full(max(n, 1), -1, np.float32), np.full(max(n, 1), -1, np.float32)
        ctx = self.el.ctx
        ctx.check(lib().svgpu_stereo_match(ctx.handle, self.er.ctx.handle, _p(self.kl), _p(self.dl), n, _p(self.kr), _p(self.dr),
                                           len(self.kr), self.focal_x_baseline_, self.true_baseline_,
                                           _p(xr), _p(dp)), "svgpu_stereo_match")
        return xr[:n].copy(), dp[:n].copy()


# ------------------------------------------------------------------------------------------- function-specific matchers
# Flat-array mirrors of the reference methods whose candidate generation and gates run on the device (include/svgpu.h,
# "function-specific matchers").  Argument names are the C ABI's; `cam` is a camera.base (its svgpu_camera carries img_bounds_).

def _f64(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float64)
    return a if shape is None else a.reshape(shape)


def _call(ctx, fn_name, args):
    ctx.check(getattr(lib(), fn_name)(ctx.handle, *args), fn_name)


class projection_flat(base):
    """match::projection's methods other than match_frame_and_landmarks, on flat arrays (match/projection.cc:95-629)."""

    def match_current_and_last_frames(self, cam, rot_cw, trans_cw, rot_lw, trans_lw, pos_w, valid, lm_desc, octave_last, angle_last,
                                      scale_factors, margin, tdesc, t_xy, t_octave, t_angle, occupied=None, t_xright=None,
                                      lm_has_observation=None, is_monocular=True, true_baseline=0.0, grid_cols=64, grid_rows=48):
        pw = _f64(pos_w, (-1, 3))
        n, sf = len(pw), _c(scale_factors, np.float32)
        td = _c(tdesc, np.uint8)
        out, num = np.full(n, -1, np.int32), C.c_int(0)
        a = [C.byref(cam.c_), _p(_f64(rot_cw)), _p(_f64(trans_cw)), _p(_f64(rot_lw)), _p(_f64(trans_lw)), int(is_monocular), true_baseline,
             n, _p(pw), _p(_c(valid, np.uint8)), _p(_c(lm_desc, np.uint8)), _p(_c(octave_last, np.int32)), _p(_c(angle_last, np.float32)),
             _p(_c(lm_has_observation, np.uint8)), len(sf), _p(sf), margin, _p(td), _p(_c(t_xy, np.float32)), _p(_c(t_octave, np.int32)),
             _p(_c(t_angle, np.float32)), len(td), _p(_c(occupied, np.uint8)), _p(_c(t_xright, np.float32)), grid_cols, grid_rows,
             int(self.check_orientation_), _p(out), C.byref(num)]
        keep = a  # noqa: F841  (the temporaries stay alive until the call returns)
        _call(self.ctx, "svgpu_match_current_and_last_frames", a)
        return out, num.value

    def match_frame_and_keyframe(self, cam, rot_cw, trans_cw, pos_w, valid, min_valid_dist, max_valid_dist, lm_desc, angle_kf, scale_factors,
                                 log_scale_factor, margin, hamm_dist_thr, tdesc, t_xy, t_octave, t_angle, occupied=None, grid_cols=64, grid_rows=48):
        pw = _f64(pos_w, (-1, 3))
        n, sf, td = len(pw), _c(scale_factors, np.float32), _c(tdesc, np.uint8)
        out, num = np.full(n, -1, np.int32), C.c_int(0)
        _call(self.ctx, "svgpu_match_frame_and_keyframe_projection",
              [C.byref(cam.c_), _p(_f64(rot_cw)), _p(_f64(trans_cw)), n, _p(pw), _p(_c(valid, np.uint8)), _p(_c(min_valid_dist, np.float32)),
               _p(_c(max_valid_dist, np.float32)), _p(_c(lm_desc, np.uint8)), _p(_c(angle_kf, np.float32)), len(sf), _p(sf), log_scale_factor,
               margin, hamm_dist_thr, _p(td), _p(_c(t_xy, np.float32)), _p(_c(t_octave, np.int32)), _p(_c(t_angle, np.float32)),
               len(td), _p(_c(occupied, np.uint8)), grid_cols, grid_rows, int(self.check_orientation_), _p(out), C.byref(num)])
        return out, num.value

    def match_by_Sim3_transform(self, cam, sim3_cw, pos_w, valid, min_valid_dist, max_valid_dist, mean_normal, lm_desc, scale_factors, log_scale_factor,
                                margin, tdesc, t_xy, t_octave, occupied=None, grid_cols=64, grid_rows=48):
        pw = _f64(pos_w, (-1, 3))
        n, sf, td = len(pw), _c(scale_factors, np.float32), _c(tdesc, np.uint8)
        out, num = np.full(n, -1, np.int32), C.c_int(0)
        _call(self.ctx, "svgpu_match_by_sim3_transform",
              [C.byref(cam.c_), _p(_f64(sim3_cw)), n, _p(pw), _p(_c(valid, np.uint8)), _p(_c(min_valid_dist, np.float32)), _p(_c(max_valid_dist, np.float32)),
               _p(_f64(mean_normal)), _p(_c(lm_desc, np.uint8)), len(sf), _p(sf), log_scale_factor, margin, _p(td),
               _p(_c(t_xy, np.float32)), _p(_c(t_octave, np.int32)), len(td), _p(_c(occupied, np.uint8)), grid_cols, grid_rows, _p(out), C.byref(num)])
        return out, num.value

    def match_keyframes_mutually(self, cam1, cam2, rot_1w, trans_1w, rot_2w, trans_2w, s_12, rot_12, trans_12, kf1, kf2, scale_factors,
                                 log_scale_factor, margin, grid_cols=64, grid_rows=48):
        """kf1 / kf2: dicts with pos_w, valid, min_valid_dist, max_valid_dist, lm_desc (the keyframe's landmarks, one per keypoint) and
        desc, xy, octave (its keypoints)."""
        sf = _c(scale_factors, np.float32)

        def side(k):
            pw = _f64(k["pos_w"], (-1, 3))
            return [len(pw), _p(pw), _p(_c(k["valid"], np.uint8)), _p(_c(k["min_valid_dist"], np.float32)), _p(_c(k["max_valid_dist"], np.float32)),
                    _p(_c(k["lm_desc"], np.uint8)), _p(_c(k["desc"], np.uint8)), _p(_c(k["xy"], np.float32)), _p(_c(k["octave"], np.int32))]
        n1, n2 = len(kf1["pos_w"]), len(kf2["pos_w"])
        m21, m12, mut, num = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32), np.full(n1, -1, np.int32), C.c_int(0)
        _call(self.ctx, "svgpu_match_keyframes_mutually",
              [C.byref(cam1.c_), C.byref(cam2.c_), _p(_f64(rot_1w)), _p(_f64(trans_1w)), _p(_f64(rot_2w)), _p(_f64(trans_2w)), s_12, _p(_f64(rot_12)),
               _p(_f64(trans_12))] + side(kf1) + side(kf2) + [len(sf), _p(sf), log_scale_factor, margin, grid_cols, grid_rows, _p(m21),
                                                             _p(m12), _p(mut), C.byref(num)])
        return m21, m12, mut, num.value


class fuse:
    """match/fuse.h: detect_duplication on flat arrays (match/fuse.cc:11-154)."""

    def __init__(self, lowe_ratio: float = 0.6, ctx: Context | None = None):
        self.lowe_ratio_ = float(lowe_ratio)
        self.ctx = ctx or Context()

    def detect_duplication(self, cam, rot_cw, trans_cw, pos_w, valid, min_valid_dist, max_valid_dist, mean_normal, lm_desc, scale_factors,
                           inv_level_sigma_sq, log_scale_factor, margin, tdesc, t_xy, t_octave, t_xright=None, do_reprojection_matching=False,
                           grid_cols=64, grid_rows=48):
        pw = _f64(pos_w, (-1, 3))
        n, sf, td = len(pw), _c(scale_factors, np.float32), _c(tdesc, np.uint8)
        out, num = np.full(n, -1, np.int32), C.c_int(0)
        _call(self.ctx, "svgpu_fuse_detect_duplication",
              [C.byref(cam.c_), _p(_f64(rot_cw)), _p(_f64(trans_cw)), n, _p(pw), _p(_c(valid, np.uint8)), _p(_c(min_valid_dist, np.float32)),
               _p(_c(max_valid_dist, np.float32)), _p(_f64(mean_normal)), _p(_c(lm_desc, np.uint8)), len(sf), _p(sf), _p(_c(inv_level_sigma_sq, np.float32)),
               log_scale_factor, margin, int(do_reprojection_matching), _p(td), _p(_c(t_xy, np.float32)), _p(_c(t_octave, np.int32)),
               _p(_c(t_xright, np.float32)), len(td), grid_cols, grid_rows, _p(out), C.byref(num)])
        return out, num.value


def reproject_to_bearing(cam, rot_cw, trans_cw, pos_w):
    """camera::*::reproject_to_bearing -> (bearing 3, valid)."""
    b, v = np.zeros(3), C.c_int(0)
    lib().svgpu_reproject_to_bearing(C.byref(cam.c_), _p(_f64(rot_cw)), _p(_f64(trans_cw)), _p(_f64(pos_w)), _p(b), C.byref(v))
    return b, bool(v.value)


def match_for_triangulation(ctx, lowe_ratio, check_orientation, desc1, angle1, octave1, bearings1, has_lm1, desc2, angle2, bearings2, has_lm2, E_12,
                            epipole_in_2, valid_epipole, scale_factors, residual_rad_thr, xright1=None, xright2=None, node1=None, node2=None):
    """robust::match_for_triangulation (node1 = node2 = None) / bow_tree::match_for_triangulation (bow_feat_vec_ node ids given)."""
    d1, d2, sf = _c(desc1, np.uint8), _c(desc2, np.uint8), _c(scale_factors, np.float32)
    out, num = np.full(len(d1), -1, np.int32), C.c_int(0)
    ctx.check(lib().svgpu_match_for_triangulation(
        ctx.handle, _p(d1), _p(_c(angle1, np.float32)), _p(_c(octave1, np.int32)), _p(_f64(bearings1)), _p(_c(has_lm1, np.uint8)), _p(_c(xright1, np.float32)),
        len(d1), _p(d2), _p(_c(angle2, np.float32)), _p(_f64(bearings2)), _p(_c(has_lm2, np.uint8)), _p(_c(xright2, np.float32)), len(d2),
        _p(_c(node1, np.int32)), _p(_c(node2, np.int32)), _p(_f64(E_12)), _p(_f64(epipole_in_2)), int(valid_epipole), _p(sf), len(sf),
        residual_rad_thr, lowe_ratio, int(check_orientation), _p(out), C.byref(num)), "svgpu_match_for_triangulation")
    return out, num.value


TRI_ACCEPTED, TRI_NO_MODE, TRI_DEPTH, TRI_REPROJECTION, TRI_SCALE, TRI_SKIPPED = 0, 1, 2, 3, 4, 255  # include/svgpu.h SVGPU_TRI_*


class svgpu_triangulate_view(C.Structure):
    """include/svgpu.h svgpu_triangulate_view."""
    _fields_ = [("cam", C.c_void_p), ("pose_cw", C.c_void_p), ("true_baseline", C.c_double), ("xy", C.c_void_p), ("octave", C.c_void_p),
                ("bearings", C.c_void_p), ("xright", C.c_void_p), ("depth", C.c_void_p), ("n", C.c_int32), ("scale_factor", C.c_float)]


def _tri_arrays(view):
    """The converted arrays of one triangulator view, by name."""
    return dict(cam=getattr(view["cam"], "c_", view["cam"]), pose=np.ascontiguousarray(np.asarray(view["pose_cw"], np.float64)[:3, :4]),
                xy=_c(view["xy"], np.float32), octave=_c(view["octave"], np.int32), bearings=_f64(view["bearings"]),
                xright=_c(view.get("xright"), np.float32), depth=_c(view.get("depth"), np.float32))


def _tri_view(view, keep, arrays=None):
    """One keyframe side of the triangulator as a dict: cam (a camera object or its svgpu_camera), pose_cw (3 x 4 or 4 x 4), true_baseline,
    xy (n x 2), octave, bearings (n x 3), xright / depth (optional), scale_factor.  `keep` holds the converted arrays alive."""
    a = _tri_arrays(view) if arrays is None else arrays
    keep.append(a)
    v = svgpu_triangulate_view()
    v.cam, v.pose_cw, v.true_baseline = C.addressof(a["cam"]), a["pose"].ctypes.data, float(view.get("true_baseline", 0.0))
    v.xy, v.octave, v.bearings, v.xright, v.depth = (None if a[k] is None else a[k].ctypes.data for k in ("xy", "octave", "bearings", "xright", "depth"))
    v.n, v.scale_factor = len(a["octave"]), float(view["scale_factor"])
    return v


def triangulate_two_views(ctx, view1, view2, scale_factors, level_sigma_sq, idx1, idx2=None, rays_parallax_deg_thr=1.0):
    """module::two_view_triangulator::triangulate for a list of matches (idx1[m], idx2[m]); idx2 = None: idx1 is matched_2_in_1, the output of
    match_for_triangulation.  Returns pos_w (M x 3), status (M bytes, TRI_*), num_accepted."""
    keep = []
    v1, v2 = _tri_view(view1, keep), _tri_view(view2, keep)
    sf, sg, i1, i2 = _c(scale_factors, np.float32), _c(level_sigma_sq, np.float32), _c(idx1, np.int32), _c(idx2, np.int32)
    m = len(i1)
    pos, st, num = np.zeros((m, 3), np.float64), np.zeros(m, np.uint8), C.c_int(0)
    ctx.check(lib().svgpu_triangulate_two_views(
        ctx.handle, v1.cam, v1.pose_cw, v1.true_baseline, v1.xy, v1.octave, v1.bearings, v1.xright, v1.depth, v1.n,
        v2.cam, v2.pose_cw, v2.true_baseline, v2.xy, v2.octave, v2.bearings, v2.xright, v2.depth, v2.n, _p(sf), _p(sg), len(sf),
        v1.scale_factor, v2.scale_factor, rays_parallax_deg_thr, _p(i1), _p(i2), m, _p(pos), _p(st), C.byref(num)),
        "svgpu_triangulate_two_views")
    return pos, st, num.value


def triangulate_two_views_batch(ctx, view1, neighbours, match_off, scale_factors, level_sigma_sq, idx1, idx2=None, rays_parallax_deg_thr=1.0):
    """The loop of mapping_module::create_new_landmarks in one launch: `view1` against every view of `neighbours`; the matches of neighbour k
    are entries match_off[k] .. match_off[k + 1] of idx1 / idx2.  Returns pos_w, status, num_accepted per neighbour."""
    keep = []
    v1 = _tri_view(view1, keep)
    k = len(neighbours)
    nb = (svgpu_triangulate_view * max(k, 1))(*[_tri_view(v, keep) for v in neighbours])
    off = _c(match_off, np.int32)
    sf, sg, i1, i2 = _c(scale_factors, np.float32), _c(level_sigma_sq, np.float32), _c(idx1, np.int32), _c(idx2, np.int32)
    m = len(i1)
    pos, st, num = np.zeros((m, 3), np.float64), np.zeros(m, np.uint8), np.zeros(max(k, 1), np.int32)
    ctx.check(lib().svgpu_triangulate_two_views_batch(ctx.handle, C.byref(v1), nb, k, _p(off), _p(sf), _p(sg), len(sf), rays_parallax_deg_thr,
                                                      _p(i1), _p(i2), _p(pos), _p(st), _p(num)), "svgpu_triangulate_two_views_batch")
    return pos, st, num[:k]


class bow_tree(base):
    """match/bow_tree.h on flat arrays: side 1 hands its landmarks over (the keyframe), side 2 receives them (frame / other keyframe);
    node ids = bow_feat_vec_ membership of every keypoint (data.bow_vocabulary.descend)."""

    def match(self, desc1, angle1, valid1, node1, desc2, angle2, node2, valid2=None, occupied2=None):
        d1, d2 = _c(desc1, np.uint8), _c(desc2, np.uint8)
        out, num = np.full(len(d1), -1, np.int32), C.c_int(0)
        self.ctx.check(lib().svgpu_bow_match(self.ctx.handle, _p(d1), _p(_c(angle1, np.float32)), _p(_c(valid1, np.uint8)), _p(_c(node1, np.int32)),
                                             len(d1), _p(d2), _p(_c(angle2, np.float32)), _p(_c(valid2, np.uint8)), _p(_c(node2, np.int32)), len(d2),
                                             _p(_c(occupied2, np.uint8)), self.lowe_ratio_, int(self.check_orientation_), _p(out),
                                             C.byref(num)), "svgpu_bow_match")
        return out, num.value

    # bow_tree.cc:169-256: matched_lms_in_frm[match[i]] = keyfrm landmark i
    match_frame_and_keyframe = match
    # bow_tree.cc:258-366 (valid2 = keypoints of keyframe 2 that hold a live landmark)
    match_keyframes = match

    def match_for_triangulation(self, **kw):
        return match_for_triangulation(self.ctx, self.lowe_ratio_, self.check_orientation_, **kw)

    def match_batch(self, side1, side2):
        """match / match_frame_and_keyframe / match_keyframes for all partners in ONE device call (svgpu_bow_match_batch).  `side1` and
        `side2` are lists of dicts with the keyword names of match(): desc, angle, valid, node (+ occupied on side 2); ONE dict instead
        of a list means that side is shared by every problem.  Returns (list of per-problem match arrays, counts)."""
        return _match_batch(self.ctx, "svgpu_bow_match_batch", side1, side2, [], [self.lowe_ratio_, int(self.check_orientation_)])

    def match_for_triangulation_batch(self, **kw):
        return match_for_triangulation_batch(self.ctx, self.lowe_ratio_, self.check_orientation_, **kw)


class svgpu_match_view(C.Structure):
    """include/svgpu.h svgpu_match_view."""
    _fields_ = [("desc", C.c_void_p), ("angle", C.c_void_p), ("valid", C.c_void_p), ("node", C.c_void_p), ("octave", C.c_void_p),
                ("bearings", C.c_void_p), ("xright", C.c_void_p), ("occupied", C.c_void_p), ("n", C.c_int)]


def _match_view(side, keep):
    """One side as a dict: desc, angle, valid (or has_lm: inverted here, as svgpu_match_for_triangulation does), node, octave, bearings,
    xright, occupied -- all but desc optional."""
    valid = side.get("valid")
    if valid is None and side.get("has_lm") is not None:
        valid = (np.asarray(side["has_lm"]) == 0).astype(np.uint8)
    a = [np.ascontiguousarray(side["desc"], np.uint8).reshape(-1, 32), _c(side.get("angle"), np.float32), _c(valid, np.uint8),
         _c(side.get("node"), np.int32), _c(side.get("octave"), np.int32), _f64(side.get("bearings")), _c(side.get("xright"), np.float32),
         _c(side.get("occupied"), np.uint8)]
    keep.append(a)
    v = svgpu_match_view()
    v.desc, v.angle, v.valid, v.node, v.octave, v.bearings, v.xright, v.occupied = (None if x is None else x.ctypes.data for x in a)
    v.n = len(a[0])
    return v


def _match_batch(ctx, fn_name, side1, side2, mid, tail):
    shared1, shared2 = isinstance(side1, dict), isinstance(side2, dict)
    l1, l2 = ([side1] if shared1 else list(side1)), ([side2] if shared2 else list(side2))
    k = max(len(l1), len(l2)) if (shared1 or shared2) else len(l1)
    if not shared1 and not shared2 and len(l1) != len(l2):
        raise ValueError("side1 and side2 must name the same number of problems")
    keep = []
    v1 = (svgpu_match_view * max(len(l1), 1))(*[_match_view(s, keep) for s in l1])
    v2 = (svgpu_match_view * max(len(l2), 1))(*[_match_view(s, keep) for s in l2])
    n1 = [v1[0 if shared1 else p].n for p in range(k)]
    out, num = np.full(max(sum(n1), 1), -1, np.int32), np.zeros(max(k, 1), np.int32)
    ctx.check(getattr(lib(), fn_name)(ctx.handle, k, v1, int(shared1), v2, int(shared2), *mid, *tail, _p(out), _p(num)), fn_name)
    off = np.concatenate([[0], np.cumsum(n1)]).astype(np.int64)
    return [out[off[p]:off[p + 1]].copy() for p in range(k)], num[:k].copy()


def match_for_triangulation_batch(ctx, lowe_ratio, check_orientation, side1, side2, E_12, epipole_in_2, valid_epipole, scale_factors, residual_rad_thr):
    """match_for_triangulation for all neighbours in ONE device call (svgpu_match_for_triangulation_batch).  Sides as in bow_tree.match_batch
    with desc, angle, octave (side 1), bearings, has_lm, xright, node; E_12 (K x 3 x 3), epipole_in_2 (K x 3), valid_epipole (K) per problem."""
    sf = _c(scale_factors, np.float32)
    E, ep, ve = _f64(E_12), _f64(epipole_in_2), _c(np.asarray(valid_epipole).astype(np.int32), np.int32)
    return _match_batch(ctx, "svgpu_match_for_triangulation_batch", side1, side2, [_p(E), _p(ep), _p(ve), _p(sf), len(sf), residual_rad_thr],
                        [lowe_ratio, int(check_orientation)])


def triangulation_matches_to_batch(matched_2_in_1_per_neighbour):
    """The (match_off, idx1, idx2) triangulate_two_views_batch takes, from the per-neighbour matched_2_in_1 arrays of
    match_for_triangulation_batch: the matched pairs of neighbour k, in side-1 index order, are entries match_off[k] .. match_off[k + 1]."""
    idx1 = [np.flatnonzero(np.asarray(m) >= 0).astype(np.int32) for m in matched_2_in_1_per_neighbour]
    idx2 = [np.asarray(m, np.int32)[i] for m, i in zip(matched_2_in_1_per_neighbour, idx1)]
    off = np.concatenate([[0], np.cumsum([len(i) for i in idx1])]).astype(np.int32)
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)  # noqa: E731
    return off, cat(idx1), cat(idx2)


def _view_pair(side, view, keep):
    """The matcher's and the triangulator's view of ONE keyframe: octave, bearings and xright are the same arrays in both."""
    a = _tri_arrays(view)
    t = _tri_view(view, keep, a)
    m = _match_view(dict(side, octave=a["octave"], bearings=a["bearings"], xright=a["xright"]), keep)
    return m, t


def new_landmarks_batch(ctx, lowe_ratio, check_orientation, side1, view1, side2, neighbours, E_12, epipole_in_2, valid_epipole, scale_factors,
                        level_sigma_sq, residual_rad_thr, active=None, rays_parallax_deg_thr=1.0):
    """The loop of mapping_module::create_new_landmarks for all neighbours in ONE device call (svgpu_new_landmarks_batch): per neighbour
    match_for_triangulation and two_view_triangulator::triangulate, with the keypoints that got a landmark leaving the queries of every later
    neighbour -- which match_for_triangulation_batch followed by triangulate_two_views_batch, two calls over independent neighbours, do not
    reproduce.  `side1` / `side2[k]` are matcher sides (desc, angle, has_lm | valid, node, xright), `view1` / `neighbours[k]` the triangulator's
    views of the same keyframes (cam, pose_cw, true_baseline, xy, octave, bearings, xright, depth, scale_factor); octave, bearings and xright are
    taken from the triangulator's view for both.  Returns a dict: matched_2_in_1 (K x n1), pos_w (K x n1 x 3), status (K x n1, TRI_*),
    num_matches, num_accepted (K each), created_by (n1: the neighbour that gave keypoint i its landmark, or -1), stats (launches, copies,
    synchronisations)."""
    from .relocalizer import call_stats
    keep = []

    def pair(side, view):
        return _view_pair(side, view, keep)
    m1, t1 = pair(side1, view1)
    k = len(neighbours)
    if len(side2) != k:
        raise ValueError("side2 and neighbours must name the same keyframes")
    both = [pair(s, v) for s, v in zip(side2, neighbours)]
    m2 = (svgpu_match_view * max(k, 1))(*[b[0] for b in both])
    t2 = (svgpu_triangulate_view * max(k, 1))(*[b[1] for b in both])
    sf, sg = _c(scale_factors, np.float32), _c(level_sigma_sq, np.float32)
    E, ep, ve = _f64(E_12), _f64(epipole_in_2), _c(np.asarray(valid_epipole).astype(np.int32), np.int32)
    act = _c(active, np.uint8)
    n1 = m1.n
    out = dict(matched_2_in_1=np.full((k, n1), -1, np.int32), pos_w=np.zeros((k, n1, 3), np.float64), status=np.full((k, n1), TRI_SKIPPED, np.uint8),
               num_matches=np.zeros(k, np.int32), num_accepted=np.zeros(k, np.int32), created_by=np.full(n1, -1, np.int32))
    st = call_stats()
    ctx.check(lib().svgpu_new_landmarks_batch(
        ctx.handle, C.byref(m1), C.byref(t1), k, m2, t2, _p(act), _p(E), _p(ep), _p(ve), _p(sf), _p(sg), len(sf), residual_rad_thr, lowe_ratio,
        int(check_orientation), rays_parallax_deg_thr, _p(out["matched_2_in_1"]), _p(out["pos_w"]), _p(out["status"]), _p(out["num_matches"]),
        _p(out["num_accepted"]), _p(out["created_by"]), C.byref(st)), "svgpu_new_landmarks_batch")
    out["stats"] = dict(launches=st.launches, copies=st.copies, synchronisations=st.synchronisations)
    return out


FUSE_OVERFLOW = 100  # include/svgpu.h SVGPU_FUSE_OVERFLOW
FUSE_NONE, FUSE_NEW_CONNECTION, FUSE_DUP_SURVIVED, FUSE_DUP_LOST, FUSE_SAME_ID, FUSE_SKIPPED = range(6)


class svgpu_fuse_keyframe(C.Structure):
    """include/svgpu.h svgpu_fuse_keyframe."""
    _fields_ = [("cam", C.c_void_p), ("rot_cw", C.c_void_p), ("trans_cw", C.c_void_p), ("desc", C.c_void_p), ("xy", C.c_void_p), ("octave", C.c_void_p),
                ("xright", C.c_void_p), ("kp_lm", C.c_void_p), ("n", C.c_int32), ("observer", C.c_int32), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32)]


class svgpu_fuse_table(C.Structure):
    """include/svgpu.h svgpu_fuse_table."""
    _fields_ = [("num_landmarks", C.c_int32), ("num_entries", C.c_int32)] + [(k, C.c_void_p) for k in (
        "pos_w", "ref_trans_wc", "ref_scale_factor", "obs_off", "obs_cap", "alive", "descriptor", "mean_normal", "min_valid_dist", "max_valid_dist",
        "has_descriptor", "has_geometry", "obs_cnt", "obs_observer", "obs_kp", "obs_desc", "obs_weight", "replaced_by")]


_FUSE_TABLE_TYPES = dict(pos_w=np.float64, ref_trans_wc=np.float64, ref_scale_factor=np.float32, obs_off=np.int32, obs_cap=np.int32, alive=np.uint8,
                         descriptor=np.uint8, mean_normal=np.float64, min_valid_dist=np.float32, max_valid_dist=np.float32, has_descriptor=np.uint8,
                         has_geometry=np.uint8, obs_cnt=np.int32, obs_observer=np.int32, obs_kp=np.int32, obs_desc=np.uint8, obs_weight=np.int32)


def fuse_landmarks_batch(ctx, keyframes, observer_rank, observer_trans_wc, table, fwd_list, bwd_list, scale_factors, inv_level_sigma_sq, log_scale_factor,
                         inv_scale_factor_last, margin=3.0, do_reprojection_matching=True, check=True, sentinel=None):
    """mapping_module::fuse_landmark_duplication for all fuse targets in ONE device call (svgpu_fuse_landmarks_batch): `keyframes[0]` is the
    current keyframe, the others the targets in order; each a dict with cam (a camera object or its svgpu_camera), rot_cw, trans_cw, desc, xy,
    octave, xright (optional), kp_lm, observer, grid_cols, grid_rows.  `table` is a dict of the svgpu_fuse_table arrays.  Nothing passed in is
    modified.  Returns a dict: status (0, or FUSE_OVERFLOW: nothing else is meaningful then), the table's in/out arrays after the call,
    replaced_by, kp_lm (a list per keyframe), best_idx / event (the forward rows, then the backward row), num_fused, stats.
    check=False returns any status instead of raising; `sentinel` (an int below 128) fills every pure output before the call, so that what a
    refused call left untouched can be seen."""
    from .relocalizer import call_stats
    keep = []
    k = len(keyframes) - 1
    recs = (svgpu_fuse_keyframe * (k + 1))()
    kp_lm = []
    for u, f in enumerate(keyframes):
        cam = getattr(f["cam"], "c_", f["cam"])
        a = dict(rot=_f64(f["rot_cw"]), trans=_f64(f["trans_cw"]), desc=np.ascontiguousarray(f["desc"], np.uint8).reshape(-1, 32), xy=_c(f["xy"], np.float32),
                 octave=_c(f["octave"], np.int32), xright=_c(f.get("xright"), np.float32), kp_lm=np.array(f["kp_lm"], np.int32, copy=True), cam=cam)
        keep.append(a)
        kp_lm.append(a["kp_lm"])
        r = recs[u]
        r.cam, r.rot_cw, r.trans_cw = C.addressof(cam), a["rot"].ctypes.data, a["trans"].ctypes.data
        r.desc, r.xy, r.octave, r.kp_lm = a["desc"].ctypes.data, a["xy"].ctypes.data, a["octave"].ctypes.data, a["kp_lm"].ctypes.data
        r.xright = None if a["xright"] is None else a["xright"].ctypes.data
        r.n, r.observer, r.grid_cols, r.grid_rows = len(a["octave"]), int(f["observer"]), int(f.get("grid_cols", 64)), int(f.get("grid_rows", 48))
    t = {key: np.array(table[key], ty, copy=True) for key, ty in _FUSE_TABLE_TYPES.items()}
    t["replaced_by"] = np.full(len(t["obs_off"]), -1, np.int32)
    tab = svgpu_fuse_table()
    tab.num_landmarks, tab.num_entries = len(t["obs_off"]), len(t["obs_observer"])
    for key, arr in t.items():
        setattr(tab, key, arr.ctypes.data)
    rank, twc = _c(observer_rank, np.int32), _f64(observer_trans_wc)
    fwd, bwd = _c(fwd_list, np.int32), _c(bwd_list, np.int32)
    sf, ils = _c(scale_factors, np.float32), _c(inv_level_sigma_sq, np.float32)
    n_out = k * len(fwd) + len(bwd)
    best, event, num = np.full(max(n_out, 1), -1, np.int32), np.zeros(max(n_out, 1), np.uint8), np.zeros(k + 1, np.int32)
    st = call_stats()
    if sentinel is not None:
        best[:], event[:], num[:], t["replaced_by"][:] = sentinel, sentinel, sentinel, sentinel
        st.launches = st.copies = st.synchronisations = sentinel
    rc = lib().svgpu_fuse_landmarks_batch(ctx.handle, k, recs, len(rank), _p(rank), _p(twc), C.byref(tab), len(fwd), _p(fwd), len(bwd), _p(bwd), len(sf),
                                          _p(sf), _p(ils), log_scale_factor, inv_scale_factor_last, margin, int(do_reprojection_matching), _p(best), _p(event),
                                          _p(num), C.byref(st))
    if check and rc != FUSE_OVERFLOW:
        ctx.check(rc, "svgpu_fuse_landmarks_batch")
    out = {key: t[key] for key in t if key not in ("pos_w", "ref_trans_wc", "ref_scale_factor", "obs_off", "obs_cap")}
    out.update(status=rc, kp_lm=kp_lm, best_idx=best[:n_out], event=event[:n_out], num_fused=num,
               stats=dict(launches=st.launches, copies=st.copies, synchronisations=st.synchronisations))
    return out
