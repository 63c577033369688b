"""solve::pnp_solver (solve/pnp_solver.cc) on the device: thin mirror of svgpu_pnp_compute_pose / svgpu_pnp_ransac[_batch]
(include/svgpu.h).  The RANSAC sample table is an argument: draw it with the engine of your choice (the reference draws it with
util::create_random_array from a std::mt19937)."""
from __future__ import annotations

import numpy as np

from ._lib import lib, ptr as _p
from .feature import Context


def compute_pose(ctx: Context, bearings, pos_w, set_off=None, gauss_newton_num_iter=10):
    """pnp_solver::compute_pose for the sets set_off[s] .. set_off[s + 1] of the n x 3 arrays (set_off = None: one set of all).
    Returns pose_cw (num_sets x 3 x 4, [R | t]) and reproj_error (num_sets)."""
    b, w = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3), np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray([0, len(b)] if set_off is None else set_off, np.int32)
    k = len(off) - 1
    pose, err = np.zeros((k, 3, 4), np.float64), np.zeros(k, np.float64)
    ctx.check(lib().svgpu_pnp_compute_pose(ctx.handle, k, _p(off), _p(b), _p(w), int(gauss_newton_num_iter), _p(pose), _p(err)), "svgpu_pnp_compute_pose")
    return pose, err


def _ransac_out(k, n, num_iter, with_hypotheses):
    out = dict(valid=np.zeros(k, np.uint8), pose_cw=np.zeros((k, 3, 4), np.float64), is_inlier=np.zeros(n, np.uint8), best_iter=np.zeros(k, np.int32))
    if with_hypotheses:
        out.update(hyp_pose=np.zeros((k, num_iter, 3, 4), np.float64), hyp_num_inliers=np.zeros((k, num_iter), np.int32), hyp_cost=np.zeros((k, num_iter), np.float64))
    return out


def pnp_ransac_batch(ctx: Context, match_off, bearings, pos_w, octaves, scale_factors, samples, min_num_inliers=10, recompute=True, gauss_newton_num_iter=10,
                     with_hypotheses=False):
    """pnp_solver::find_via_ransac for the problems match_off[p] .. match_off[p + 1]; samples: num_problems x num_iter x 4 indices local to their
    problem.  Returns a dict: valid, pose_cw, is_inlier, best_iter (and hyp_pose, hyp_num_inliers, hyp_cost with with_hypotheses)."""
    off = np.ascontiguousarray(match_off, np.int32)
    k = len(off) - 1
    b, w = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3), np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    o, sf = np.ascontiguousarray(octaves, np.int32), np.ascontiguousarray(scale_factors, np.float32)
    s = np.ascontiguousarray(samples, np.uint32).reshape(max(k, 0), -1, 4) if k > 0 else np.zeros((0, 0, 4), np.uint32)
    num_iter = s.shape[1]
    out = _ransac_out(max(k, 0), len(b), num_iter, with_hypotheses)
    ctx.check(lib().svgpu_pnp_ransac_batch(ctx.handle, k, _p(off), _p(b), _p(w), _p(o), _p(sf), len(sf), int(min_num_inliers), num_iter, _p(s), int(bool(recompute)),
                                           int(gauss_newton_num_iter), _p(out["valid"]), _p(out["pose_cw"]), _p(out["is_inlier"]), _p(out["best_iter"]),
                                           _p(out.get("hyp_pose")), _p(out.get("hyp_num_inliers")), _p(out.get("hyp_cost"))), "svgpu_pnp_ransac_batch")
    return out


def pnp_ransac(ctx: Context, bearings, pos_w, octaves, scale_factors, samples, min_num_inliers=10, recompute=True, gauss_newton_num_iter=10,
               with_hypotheses=False):
    """One problem (svgpu_pnp_ransac): samples is num_iter x 4.  Same dict as pnp_ransac_batch, with a leading axis of one problem."""
    b, w = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3), np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    o, sf = np.ascontiguousarray(octaves, np.int32), np.ascontiguousarray(scale_factors, np.float32)
    s = np.ascontiguousarray(samples, np.uint32).reshape(-1, 4)
    out = _ransac_out(1, len(b), len(s), with_hypotheses)
    ctx.check(lib().svgpu_pnp_ransac(ctx.handle, _p(b), _p(w), _p(o), len(b), _p(sf), len(sf), int(min_num_inliers), len(s), _p(s), int(bool(recompute)),
                                     int(gauss_newton_num_iter), _p(out["valid"]), _p(out["pose_cw"]), _p(out["is_inlier"]), _p(out["best_iter"]),
                                     _p(out.get("hyp_pose")), _p(out.get("hyp_num_inliers")), _p(out.get("hyp_cost"))), "svgpu_pnp_ransac")
    return out

