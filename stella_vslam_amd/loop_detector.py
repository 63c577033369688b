"""module/loop_detector.h on flat arrays: the middle of select_loop_candidate_via_Sim3 (module/loop_detector.cc:537-587) -- scale, mutual
match, edge gather and Sim3 optimisation -- for all candidates in one device call (svgpu_loop_sim3_batch, include/svgpu.h).  The
arguments carry the C ABI's names."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, ptr as _p
from .optimize import _Camera, _Sim3OptStats
from .relocalizer import call_stats

NO_SCALE, FEW_INLIERS = 1, 2  # SVGPU_LOOP_NO_SCALE, SVGPU_LOOP_FEW_INLIERS


def _c(a, t, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, t)
    return a if shape is None else a.reshape(shape)


def _cam_bytes(cam):
    c = cam.c_ if hasattr(cam, "c_") else cam
    b = bytes(c)
    if len(b) != C.sizeof(_Camera):
        raise ValueError("validate_sim3_batch: a camera that is not laid out as svgpu_camera")
    return b


def validate_sim3_batch(ctx, cam1, cam2s, *, pose_1w, desc1, xy1, octave1, pos_w1, has_lm1, min_valid1, max_valid1, lm_desc1, scale_factors,
                        inv_level_sigma_sq, log_scale_factor, pose_2w, kf2_off, desc2, xy2, octave2, pos_w2, has_lm2, min_valid2, max_valid2,
                        lm_desc2, pose_1w_in_cand, rot_12, trans_12, sim3_12, prior_state, prior_idx2, prior_pos_w, active=None,
                        scale_12_in=None, margin=7.5, chi_sq=10.0, fix_scale=False, num_iter=10, min_num_inliers=20, grid_cols=64, grid_rows=48,
                        want_stats=False):
    """Scale, mutual match and Sim3 optimisation of the K candidates that survived the pose refinement.  cam1 / cam2s[p]: a camera.base or
    anything laid out as svgpu_camera.  Keyframe 1 (the current keyframe): pose_1w (12), its n1 keypoints desc1 / xy1 / octave1 and one
    landmark slot per keypoint pos_w1 / has_lm1 / min_valid1 / max_valid1 / lm_desc1.  Candidate p: pose_2w[p] (12), the entries
    kf2_off[p] .. kf2_off[p + 1] of the keyframe-2 arrays, pose_1w_in_cand[p] (12), rot_12[p] (9), trans_12[p] (3), sim3_12[p] (8, the
    scale entry ignored) and the prior matches prior_state / prior_idx2 / prior_pos_w (K x n1).  Returns a dict: status (K; 0 accepted,
    NO_SCALE, FEW_INLIERS, -1 inactive), scale_12 (K), matched_2_in_1 / mutual_2_in_1 (K, n1), matched_1_in_2 (by kf2_off), num_mutual,
    num_edges, num_inliers (K), edge_idx1 / edge_idx2 / edge_status (K, n1), sim3_12_out (K, 8), the optimiser's per-candidate stats
    (lm_iterations, lm_trials, early_return, num_survivors, first_chi2, last_chi2, lambda_final) and, with want_stats, stats =
    (launches, copies, synchronisations)."""
    xy, off = _c(xy1, np.float32, (-1, 2)), _c(kf2_off, np.int32, (-1,))
    n1, K = len(xy), len(off) - 1
    sf, w = _c(scale_factors, np.float32), _c(inv_level_sigma_sq, np.float32)
    x2 = _c(xy2, np.float32, (-1, 2))
    N2 = len(x2)
    ps, pi, pp = _c(prior_state, np.uint8), _c(prior_idx2, np.int32), _c(prior_pos_w, np.float64)
    if (K < 0 or len(cam2s) != K or len(sf) != len(w) or (K > 0 and off[-1] != N2) or ps.size != K * n1 or pi.size != K * n1 or pp.size != K * n1 * 3
            or np.size(pose_2w) != K * 12 or np.size(pose_1w_in_cand) != K * 12 or np.size(rot_12) != K * 9 or np.size(trans_12) != K * 3
            or np.size(sim3_12) != K * 8 or (scale_12_in is not None and np.size(scale_12_in) != K) or (active is not None and np.size(active) != K)):
        raise ValueError("validate_sim3_batch: array lengths disagree")
    cams = (C.c_char * (C.sizeof(_Camera) * max(K, 1))).from_buffer_copy(b"".join(_cam_bytes(c) for c in cam2s).ljust(C.sizeof(_Camera) * max(K, 1), b"\0"))
    cam1b = (C.c_char * C.sizeof(_Camera)).from_buffer_copy(_cam_bytes(cam1))
    Kn, E = max(K, 1), max(K * n1, 1)
    out = dict(status=np.zeros(Kn, np.int32), scale_12=np.zeros(Kn, np.float32), matched_2_in_1=np.full(E, -1, np.int32),
               matched_1_in_2=np.full(max(N2, 1), -1, np.int32), mutual_2_in_1=np.full(E, -1, np.int32), num_mutual=np.zeros(Kn, np.int32),
               edge_idx1=np.full(E, -1, np.int32), edge_idx2=np.full(E, -1, np.int32), num_edges=np.zeros(Kn, np.int32),
               edge_status=np.zeros(E, np.uint8), sim3_12_out=np.zeros((Kn, 8)), num_inliers=np.zeros(Kn, np.int32))
    ost = (_Sim3OptStats * Kn)()
    st = call_stats()
    ctx.check(lib().svgpu_loop_sim3_batch(
        ctx.handle, C.cast(cam1b, C.c_void_p), _p(_c(pose_1w, np.float64, (12,))), n1, _p(_c(desc1, np.uint8)), _p(xy), _p(_c(octave1, np.int32)),
        _p(_c(pos_w1, np.float64)), _p(_c(has_lm1, np.uint8)), _p(_c(min_valid1, np.float32)), _p(_c(max_valid1, np.float32)), _p(_c(lm_desc1, np.uint8)),
        len(sf), _p(sf), _p(w), log_scale_factor, grid_cols, grid_rows, K, C.cast(cams, C.c_void_p), _p(_c(pose_2w, np.float64)), _p(off),
        _p(_c(desc2, np.uint8)), _p(x2), _p(_c(octave2, np.int32)), _p(_c(pos_w2, np.float64)), _p(_c(has_lm2, np.uint8)), _p(_c(min_valid2, np.float32)),
        _p(_c(max_valid2, np.float32)), _p(_c(lm_desc2, np.uint8)), _p(_c(pose_1w_in_cand, np.float64)), _p(_c(rot_12, np.float64)),
        _p(_c(trans_12, np.float64)), _p(_c(sim3_12, np.float64)), _p(_c(active, np.uint8)), _p(ps), _p(pi), _p(pp), _p(_c(scale_12_in, np.float32)),
        margin, chi_sq, int(bool(fix_scale)), int(num_iter), int(min_num_inliers), _p(out["status"]), _p(out["scale_12"]), _p(out["matched_2_in_1"]),
        _p(out["matched_1_in_2"]), _p(out["mutual_2_in_1"]), _p(out["num_mutual"]), _p(out["edge_idx1"]), _p(out["edge_idx2"]), _p(out["num_edges"]),
        _p(out["edge_status"]), _p(out["sim3_12_out"]), _p(out["num_inliers"]), C.cast(ost, C.c_void_p), C.byref(st)), "svgpu_loop_sim3_batch")
    for k in ("status", "scale_12", "num_mutual", "num_edges", "sim3_12_out", "num_inliers"):
        out[k] = out[k][:K].copy()
    for k in ("matched_2_in_1", "mutual_2_in_1", "edge_idx1", "edge_idx2", "edge_status"):
        out[k] = out[k][:K * n1].reshape(K, n1).copy()
    out["matched_1_in_2"] = out["matched_1_in_2"][:N2].copy()
    for k, _ in _Sim3OptStats._fields_:
        out[k] = np.array([np.array(getattr(ost[p], k)) for p in range(K)])
    if want_stats:
        out["stats"] = (st.launches, st.copies, st.synchronisations)
    return out
