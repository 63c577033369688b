"""module/relocalizer.h on flat arrays: refine_pose for all candidates of a relocalisation in one device call
(svgpu_reloc_refine_batch, include/svgpu.h), and the whole of reloc_by_candidate behind the BoW matcher -- PnP, pose optimisation,
bookkeeping, refine_pose -- in one (svgpu_reloc_solve_batch).  The arguments carry the C ABI's names."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, ptr as _p


class call_stats(C.Structure):
    """svgpu_call_stats: what one call issued"""
    _fields_ = [("launches", C.c_int32), ("copies", C.c_int32), ("synchronisations", C.c_int32)]


RELOC_PNP_FAILED, RELOC_OPTIMIZE_FAILED = -2, -3  # SVGPU_RELOC_PNP_FAILED, SVGPU_RELOC_OPTIMIZE_FAILED


def _c(a, t, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, t)
    return a if shape is None else a.reshape(shape)


def refine_pose_batch(ctx, cam, *, tdesc, t_xy, t_octave, t_angle, t_xright, scale_factors, inv_level_sigma_sq, log_scale_factor, intrinsics,
                      pose_cw, n_already_found, frame_has_lm, frame_lm_pos_w, kf_off, pos_w, valid, min_valid_dist, max_valid_dist, lm_desc,
                      angle_kf, margin=(10.0, 3.0), hamm_dist_thr=(100, 64), min_num_valid_obs=50, active=None, check_orientation=True,
                      num_trials_robust=2, num_trials=2, num_each_iter=10, reset_stop_flag_each_round=False, grid_cols=64, grid_rows=48,
                      want_stats=False):
    """relocalizer::refine_pose (module/relocalizer.cc:236-297) for the K candidates that survived optimize_pose.  `cam` is a camera.base or
    anything laid out as svgpu_camera.  Per candidate p: pose_cw[p] (12), n_already_found[p], frame_has_lm[p] (nt) / frame_lm_pos_w[p]
    (nt x 3) = the frame's landmarks after optimize_pose, and the keyframe's entries kf_off[p] .. kf_off[p + 1] of pos_w / valid /
    min_valid_dist / max_valid_dist / lm_desc / angle_kf.  Returns a dict: status (K; 0 accepted, 1 + s failed the count test of stage s,
    1 + stages failed the final test, -1 inactive), pose_out (K, 12), match_kf / match_stage (per entry), outlier (K, nt), num_found /
    num_valid (K, stages), lm_iterations (K) and, with want_stats, stats = (launches, copies, synchronisations)."""
    td, xy = _c(tdesc, np.uint8, (-1, 32)), _c(t_xy, np.float32, (-1, 2))
    nt = len(xy)
    off = _c(kf_off, np.int32, (-1,))
    K = len(off) - 1
    sf, w = _c(scale_factors, np.float32), _c(inv_level_sigma_sq, np.float32)
    mg, thr = _c(margin, np.float32, (-1,)), _c(hamm_dist_thr, np.int32, (-1,))
    S = len(mg)
    pose = _c(pose_cw, np.float64, (-1, 12))
    pw = _c(pos_w, np.float64, (-1, 3))
    N = len(pw)
    has, lmp = _c(frame_has_lm, np.uint8, (-1, nt) if nt else None), _c(frame_lm_pos_w, np.float64)
    if (K < 0 or len(thr) != S or len(sf) != len(w) or len(pose) != K or len(td) != nt or (K > 0 and off[-1] != N)
            or (has is not None and has.size != K * nt) or (lmp is not None and lmp.size != K * nt * 3)):
        raise ValueError("refine_pose_batch: array lengths disagree")
    out = dict(status=np.zeros(max(K, 1), np.int32), pose_out=np.zeros((max(K, 1), 12)), match_kf=np.full(max(N, 1), -1, np.int32),
               match_stage=np.full(max(N, 1), -1, np.int32), outlier=np.zeros((max(K, 1), max(nt, 1)), np.uint8),
               num_found=np.zeros((max(K, 1), S), np.int32), num_valid=np.zeros((max(K, 1), S), np.int32), lm_iterations=np.zeros(max(K, 1), np.int32))
    flat_outl = np.zeros(max(K * nt, 1), np.uint8)
    st = call_stats()
    camp = C.byref(cam.c_) if hasattr(cam, "c_") else C.byref(cam)
    ctx.check(lib().svgpu_reloc_refine_batch(
        ctx.handle, camp, _p(td), _p(xy), _p(_c(t_octave, np.int32)), _p(_c(t_angle, np.float32)), _p(_c(t_xright, np.float32)), nt, grid_cols, grid_rows,
        len(sf), _p(sf), _p(w), log_scale_factor, _p(_c(intrinsics, np.float64, (5,))), num_trials_robust, num_trials, num_each_iter,
        int(reset_stop_flag_each_round), int(check_orientation), K, _p(_c(active, np.uint8)), _p(pose), _p(_c(n_already_found, np.int32)), _p(has), _p(lmp),
        _p(off), _p(pw), _p(_c(valid, np.uint8)), _p(_c(min_valid_dist, np.float32)), _p(_c(max_valid_dist, np.float32)), _p(_c(lm_desc, np.uint8)),
        _p(_c(angle_kf, np.float32)), S, _p(mg), _p(thr), int(min_num_valid_obs), _p(out["status"]), _p(out["pose_out"]), _p(out["match_kf"]),
        _p(out["match_stage"]), _p(flat_outl), _p(out["num_found"]), _p(out["num_valid"]), _p(out["lm_iterations"]), C.byref(st)),
        "svgpu_reloc_refine_batch")
    out["outlier"] = flat_outl[:K * nt].reshape(K, nt).copy()
    for k in ("status", "pose_out", "num_found", "num_valid", "lm_iterations"):
        out[k] = out[k][:K].copy()
    out["match_kf"], out["match_stage"] = out["match_kf"][:N].copy(), out["match_stage"][:N].copy()
    if want_stats:
        out["stats"] = (st.launches, st.copies, st.synchronisations)
    return out


def solve_batch(ctx, cam, *, tdesc, t_xy, t_octave, t_angle, t_xright, t_bearings, scale_factors, inv_level_sigma_sq, log_scale_factor, intrinsics,
                match_off, m_keypt, m_pos_w, m_kf_entry, samples, kf_off, pos_w, valid, min_valid_dist, max_valid_dist, lm_desc, angle_kf,
                min_num_inliers=10, recompute=False, gauss_newton_num_iter=10, min_num_opt_valid_obs=10, margin=(10.0, 3.0), hamm_dist_thr=(100, 64),
                min_num_valid_obs=50, active=None, check_orientation=True, num_trials_robust=2, num_trials=2, num_each_iter=10,
                reset_stop_flag_each_round=False, grid_cols=64, grid_rows=48, want_stats=False):
    """relocalizer::reloc_by_candidate (module/relocalizer.cc:93-132) behind the BoW matcher for K candidates at once: PnP RANSAC over the
    candidate's 2D-3D matches (entries match_off[p] .. match_off[p + 1] of m_keypt / m_pos_w / m_kf_entry; samples (K, num_iter, 4)) ->
    pose optimisation over the inliers -> bookkeeping -> refine_pose over the keyframe's entries.  Returns a dict: status (K; 0 accepted,
    -1 inactive, RELOC_PNP_FAILED, RELOC_OPTIMIZE_FAILED, else as refine_pose_batch), pnp_valid / pnp_pose_cw / best_iter (K), is_inlier
    (per match), opt_pose / opt_num_valid (K), opt_outlier (per match), every output of refine_pose_batch and, with want_stats, stats."""
    td, xy = _c(tdesc, np.uint8, (-1, 32)), _c(t_xy, np.float32, (-1, 2))
    nt = len(xy)
    off, moff = _c(kf_off, np.int32, (-1,)), _c(match_off, np.int32, (-1,))
    K = len(off) - 1
    sf, w = _c(scale_factors, np.float32), _c(inv_level_sigma_sq, np.float32)
    mg, thr = _c(margin, np.float32, (-1,)), _c(hamm_dist_thr, np.int32, (-1,))
    S = len(mg)
    pw, mpw = _c(pos_w, np.float64, (-1, 3)), _c(m_pos_w, np.float64, (-1, 3))
    N, M = len(pw), len(mpw)
    mk, me = _c(m_keypt, np.int32, (-1,)), _c(m_kf_entry, np.int32, (-1,))
    smp = _c(samples, np.uint32, (K, -1, 4) if K > 0 else None)
    brg = _c(t_bearings, np.float64, (-1, 3))
    if (K < 0 or len(thr) != S or len(sf) != len(w) or len(moff) != K + 1 or len(td) != nt or len(brg) != nt or (K > 0 and (off[-1] != N or moff[-1] != M))
            or len(mk) != M or len(me) != M):
        raise ValueError("solve_batch: array lengths disagree")
    num_iter = smp.shape[1] if K > 0 else 0
    k1, n1, m1 = max(K, 1), max(N, 1), max(M, 1)
    out = dict(status=np.zeros(k1, np.int32), pnp_valid=np.zeros(k1, np.uint8), pnp_pose_cw=np.zeros((k1, 12)), is_inlier=np.zeros(m1, np.uint8),
               best_iter=np.zeros(k1, np.int32), opt_pose=np.zeros((k1, 12)), opt_outlier=np.zeros(m1, np.uint8), opt_num_valid=np.zeros(k1, np.int32),
               pose_out=np.zeros((k1, 12)), match_kf=np.full(n1, -1, np.int32), match_stage=np.full(n1, -1, np.int32),
               outlier=np.zeros(max(K * nt, 1), np.uint8), num_found=np.zeros((k1, S), np.int32), num_valid=np.zeros((k1, S), np.int32),
               lm_iterations=np.zeros(k1, np.int32))
    st = call_stats()
    camp = C.byref(cam.c_) if hasattr(cam, "c_") else C.byref(cam)
    ctx.check(lib().svgpu_reloc_solve_batch(
        ctx.handle, camp, _p(td), _p(xy), _p(_c(t_octave, np.int32)), _p(_c(t_angle, np.float32)), _p(_c(t_xright, np.float32)), _p(brg), nt, grid_cols,
        grid_rows, len(sf), _p(sf), _p(w), log_scale_factor, _p(_c(intrinsics, np.float64, (5,))), num_trials_robust, num_trials, num_each_iter,
        int(reset_stop_flag_each_round), int(check_orientation), K, _p(_c(active, np.uint8)), _p(moff), _p(mk), _p(mpw), _p(me), int(min_num_inliers),
        num_iter, _p(smp), int(recompute), int(gauss_newton_num_iter), int(min_num_opt_valid_obs), _p(off), _p(pw), _p(_c(valid, np.uint8)),
        _p(_c(min_valid_dist, np.float32)), _p(_c(max_valid_dist, np.float32)), _p(_c(lm_desc, np.uint8)), _p(_c(angle_kf, np.float32)), S, _p(mg), _p(thr),
        int(min_num_valid_obs), _p(out["status"]), _p(out["pnp_valid"]), _p(out["pnp_pose_cw"]), _p(out["is_inlier"]), _p(out["best_iter"]),
        _p(out["opt_pose"]), _p(out["opt_outlier"]), _p(out["opt_num_valid"]), _p(out["pose_out"]), _p(out["match_kf"]), _p(out["match_stage"]),
        _p(out["outlier"]), _p(out["num_found"]), _p(out["num_valid"]), _p(out["lm_iterations"]), C.byref(st)), "svgpu_reloc_solve_batch")
    out["outlier"] = out["outlier"][:K * nt].reshape(K, nt).copy()
    for k in ("status", "pnp_valid", "pnp_pose_cw", "best_iter", "opt_pose", "opt_num_valid", "pose_out", "num_found", "num_valid", "lm_iterations"):
        out[k] = out[k][:K].copy()
    for k in ("is_inlier", "opt_outlier"):
        out[k] = out[k][:M].copy()
    out["match_kf"], out["match_stage"] = out["match_kf"][:N].copy(), out["match_stage"][:N].copy()
    if want_stats:
        out["stats"] = (st.launches, st.copies, st.synchronisations)
    return out
