"""Python mirror of stella_vslam::optimize::local_bundle_adjuster over the C ABI.

Reference interface: optimize/local_bundle_adjuster.h:15-24 -- optimize(map_db, curr_keyfrm, force_stop_flag);
created by local_bundle_adjuster_factory (backend "g2o" / "gtsam"; this one registers as "hip").  The object
graph gather (local_bundle_adjuster_g2o.cc:38-147) and the write-back (:352-430) are host-side steps of the C++
adaptor (stella_vslam_amd/host/drop_in/flat_optimizers.h); the flat problem they exchange is what
`optimize_flat` takes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, ptr as _p
from .feature import Context


class _BaProblem(C.Structure):
    _fields_ = [("num_poses", C.c_int32), ("num_points", C.c_int32), ("num_obs", C.c_int32),
                ("pose_cw", C.c_void_p), ("pose_fixed", C.c_void_p), ("points", C.c_void_p), ("point_fixed", C.c_void_p),
                ("obs_pose", C.c_void_p), ("obs_point", C.c_void_p), ("obs_uvr", C.c_void_p),
                ("obs_inv_sigma_sq", C.c_void_p), ("obs_huber_delta", C.c_void_p), ("intrinsics", C.c_void_p),
                ("num_first_iter", C.c_int32), ("num_second_iter", C.c_int32), ("gain_threshold", C.c_double)]


class _BaStats(C.Structure):
    _fields_ = [("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("iters_stage1", C.c_int32),
                ("iters_stage2", C.c_int32), ("stage2_entered", C.c_int32), ("num_gated", C.c_int32),
                ("lm_trials", C.c_int32), ("cholesky_failures", C.c_int32), ("lambda_final", C.c_double),
                ("stopped_by_terminate_action", C.c_int32), ("pcg_iterations", C.c_int32)]


def partition_keyframe_segments(scene: dict, world: int):
    """svgpu_ba_partition_keyframe_segments: landmark -> rank over the keyframe segments the `world`-rank solve will cut (host only).
    Returns (landmark_rank int32[L], info dict)."""
    a = lambda k, t: np.ascontiguousarray(scene[k], t)
    pose, pts = a("pose_cw", np.float64), a("points", np.float64)
    keep = [a("pose_fixed", np.uint8), a("obs_pose", np.int32), a("obs_point", np.int32)]
    pf = scene.get("point_fixed")
    pf = None if pf is None else np.ascontiguousarray(pf, np.uint8)
    ptr = lambda x: None if x is None else x.ctypes.data
    prob = _BaProblem(len(pose), len(pts), len(keep[1]), ptr(pose), ptr(keep[0]), ptr(pts), ptr(pf), ptr(keep[1]), ptr(keep[2]), None, None, None, None, 0, 0, 0.0)
    ranks, info = np.zeros(max(len(pts), 1), np.int32), np.zeros(12, np.int32)
    rc = lib().svgpu_ba_partition_keyframe_segments(C.byref(prob), int(world), _p(ranks), _p(info))
    if rc:
        raise RuntimeError(f"svgpu_ba_partition_keyframe_segments failed: {rc}")
    keys = ("segmented", "jobs", "cuts", "separator_keyframes", "landmarks_on_separators", "landmarks_on_separators_only", "free_keyframes", "kept_blocks", "separator_blocks", "job_exchange_doubles")
    return ranks[:len(pts)], {k: int(v) for k, v in zip(keys, info)}


def local_bundle_adjuster_factory_create(backend: str = "hip", **kw):
    """optimize/local_bundle_adjuster_factory.h:17-32 -- the backend switch."""
    if backend != "hip":
        raise RuntimeError(f"Invalid backend: {backend} (this build provides 'hip' only)")
    return local_bundle_adjuster(**kw)


SOLVER_AUTO, SOLVER_CHOLESKY, SOLVER_PCG, SOLVER_DENSE, SOLVER_PCG_MULTI, SOLVER_ENVELOPE, SOLVER_CHOLESKY_MFMA = 0, 1, 2, 3, 4, 6, 7  # svgpu_ba_solver


class local_bundle_adjuster:
    def __init__(self, num_first_iter: int = 5, num_second_iter: int = 10, ctx: Context | None = None):
        self.num_first_iter_ = num_first_iter
        self.num_second_iter_ = num_second_iter
        self.ctx = ctx or Context()

    def set_solver(self, solver: int = SOLVER_AUTO, pcg_tolerance: float = 1e-10, pcg_max_iterations: int = 0):
        """Linear solver of the reduced camera system (svgpu_ba_set_solver): on-chip LL^T / block-Jacobi PCG / dense LL^T in global memory / block envelope Cholesky."""
        self.ctx.check(lib().svgpu_ba_set_solver(self.ctx.handle, int(solver), pcg_tolerance, int(pcg_max_iterations)),
                       "svgpu_ba_set_solver")
        return self

    def last_envelope_plan(self) -> dict:
        """How the context's last envelope factorisation was planned (svgpu_ba_last_envelope_plan)."""
        info = np.zeros(8, np.int32)
        self.ctx.check(lib().svgpu_ba_last_envelope_plan(self.ctx.handle, _p(info)), "svgpu_ba_last_envelope_plan")
        return dict(kind=("one-sided", "two-sided", "segmented")[int(info[0])], rows=int(info[1]), widest_column=int(info[2]), cuts=int(info[3]),
                    jobs=int(info[4]), jobs_local=int(info[5]), separator_rows=int(info[6]), longest_job=int(info[7]))

    def last_solver(self) -> str:
        """Which solver the last stage of the context's last call resolved to (svgpu_ba_last_solver); "pcg_lds" is the PCG inside one workgroup's LDS."""
        code = C.c_int(-1)
        self.ctx.check(lib().svgpu_ba_last_solver(self.ctx.handle, C.byref(code)), "svgpu_ba_last_solver")
        return {-1: "none", SOLVER_CHOLESKY: "cholesky", SOLVER_DENSE: "dense", SOLVER_PCG_MULTI: "pcg_multi", 5: "pcg_lds", SOLVER_ENVELOPE: "envelope"}[code.value]

    def last_exchange(self) -> dict:
        """What the context's last sharded solve all-reduced (svgpu_ba_last_exchange); bytes are payload per rank."""
        info = np.zeros(10, np.int64)
        self.ctx.check(lib().svgpu_ba_last_exchange(self.ctx.handle, _p(info)), "svgpu_ba_last_exchange")
        trials, lins = max(int(info[8]), 1), max(int(info[9]), 1)
        per_trial = (int(info[3]) + int(info[4]) + int(info[5]) + int(info[6])) / trials + int(info[2]) / lins
        return dict(mode=("none", "whole reduced system", "keyframe segments")[int(info[0])], setup_bytes=int(info[1]), pose_block_bytes=int(info[2]),
                    reduced_system_bytes=int(info[3]), separator_bytes=int(info[4]), solution_bytes=int(info[5]), sums_bytes=int(info[6]),
                    allreduce_calls=int(info[7]), trials=int(info[8]), linearisations=int(info[9]), bytes_per_trial=per_trial)

    def optimize_global_flat(self, scene: dict, num_iter: int = 10, force_stop_flag: np.ndarray | None = None, gain_threshold: float = 1e-3):
        """global_bundle_adjuster core: one LM run of `num_iter` iterations over the whole graph (no outlier stage)."""
        saved = self.num_first_iter_
        self.num_first_iter_ = num_iter
        try:
            return self.optimize_flat(scene, force_stop_flag, gain_threshold, _global=True)
        finally:
            self.num_first_iter_ = saved

    def optimize_flat_sharded(self, shard: dict, rank: int, world: int, allreduce_cb=None, force_stop_flag: np.ndarray | None = None,
                              gain_threshold: float = 1e-3):
        """Multi-GPU variant: `shard` holds this rank's observations (distributed.shard_by_landmark) and the complete
        pose / point arrays; `allreduce_cb` is a svgpu_allreduce_fn (distributed.make_allreduce_callback) or None = the
        context's own RCCL communicator (distributed.init_comm)."""
        return self.optimize_flat(shard, force_stop_flag, gain_threshold, _sharded=(rank, world, allreduce_cb))

    def optimize_global_flat_sharded(self, shard: dict, rank: int, world: int, allreduce_cb=None, num_iter: int = 10,
                                     force_stop_flag: np.ndarray | None = None, gain_threshold: float = 1e-3):
        """svgpu_global_ba_sharded: the single-stage global-BA run over landmark shards."""
        saved = self.num_first_iter_
        self.num_first_iter_ = num_iter
        try:
            return self.optimize_flat(shard, force_stop_flag, gain_threshold, _sharded=(rank, world, allreduce_cb), _global=True)
        finally:
            self.num_first_iter_ = saved

    def optimize_flat(self, scene: dict, force_stop_flag: np.ndarray | None = None, gain_threshold: float = 1e-3, _sharded=None,
                      _global=False):
        """scene keys: pose_cw (P,12) f64, pose_fixed (P) u8, points (L,3) f64, [point_fixed (L) u8], obs_pose / obs_point (E) i32,
        obs_uvr (E,3) f32, obs_inv_sigma_sq (E) f32, obs_huber (E) f32, intr (P,5) f64.
        force_stop_flag: None or a writable uint8[1] (the caller's abort flag; may be SET by the terminate rule)."""
        a = lambda k, t: np.ascontiguousarray(scene[k], t)
        pose, pts = a("pose_cw", np.float64), a("points", np.float64)
        keep = [pose, pts, a("pose_fixed", np.uint8), a("obs_pose", np.int32), a("obs_point", np.int32), a("obs_uvr", np.float32),
                a("obs_inv_sigma_sq", np.float32), a("obs_huber", np.float32), a("intr", np.float64)]
        pf = scene.get("point_fixed")
        pf = None if pf is None else np.ascontiguousarray(pf, np.uint8)
        P, L, E = len(pose), len(pts), len(keep[3])
        ptr = lambda x: None if x is None else x.ctypes.data
        prob = _BaProblem(P, L, E, ptr(pose), ptr(keep[2]), ptr(pts), ptr(pf), ptr(keep[3]), ptr(keep[4]), ptr(keep[5]),
                          ptr(keep[6]), ptr(keep[7]), ptr(keep[8]), self.num_first_iter_, self.num_second_iter_, gain_threshold)
        pose_out, pts_out = np.zeros_like(pose), np.zeros_like(pts)
        outl = np.zeros(1 if _global else max(E, 1), np.uint8)  # (the global adjuster has no outlier list: no 10 MB of flags to fault in and copy at 9.6 M observations)
        st = _BaStats()
        stop = _p(force_stop_flag)
        outs = (_p(pose_out), _p(pts_out), _p(outl), C.byref(st))
        if _global and _sharded is not None:
            rank, world, cb = _sharded
            rc = lib().svgpu_global_ba_sharded(self.ctx.handle, C.byref(prob), rank, world, cb, None, stop, outs[0], outs[1], outs[3])
        elif _global:
            rc = lib().svgpu_global_ba(self.ctx.handle, C.byref(prob), stop, outs[0], outs[1], outs[3])
        elif _sharded is None:
            rc = lib().svgpu_local_ba(self.ctx.handle, C.byref(prob), stop, *outs)
        else:
            rank, world, cb = _sharded
            rc = lib().svgpu_local_ba_sharded(self.ctx.handle, C.byref(prob), rank, world, cb, None, stop, *outs)
        self.ctx.check(rc, "svgpu_local_ba", ok=(0, 7))
        return dict(rc=rc, pose_cw=pose_out, points=pts_out, outlier=(np.zeros(0, np.uint8) if _global else outl[:E].copy()),
                    stats={f: getattr(st, f) for f, _ in _BaStats._fields_})


class pose_optimizer:
    """optimize/pose_optimizer.h (g2o backend defaults of pose_optimizer_factory.h:18-26): motion-only BA of one frame."""

    def __init__(self, num_trials_robust: int = 2, num_trials: int = 2, num_each_iter: int = 10, ctx: Context | None = None,
                 reset_stop_flag_each_round: bool = False):
        self.num_trials_robust_, self.num_trials_, self.num_each_iter_ = num_trials_robust, num_trials, num_each_iter
        self.reset_stop_flag_each_round_ = reset_stop_flag_each_round
        self.ctx = ctx or Context()

    def optimize_flat(self, pose_cw, pos_w, uvr, inv_sigma_sq, huber, intr):
        """Returns (num_valid_obs, optimized pose 3x4 flat, outlier_flags, lm_iterations)."""
        pose = np.ascontiguousarray(pose_cw, np.float64).reshape(12)
        pw, uv = np.ascontiguousarray(pos_w, np.float64), np.ascontiguousarray(uvr, np.float32)
        w, hb = np.ascontiguousarray(inv_sigma_sq, np.float32), np.ascontiguousarray(huber, np.float32)
        K = np.ascontiguousarray(intr, np.float64).reshape(5)
        n = len(pw)
        out, outl = np.zeros(12), np.zeros(max(n, 1), np.uint8)
        nv, it = C.c_int(0), C.c_int(0)
        self.ctx.check(lib().svgpu_pose_optimize(self.ctx.handle, _p(pose), n, _p(pw), _p(uv), _p(w), _p(hb), _p(K), self.num_trials_robust_,
                                                 self.num_trials_, self.num_each_iter_, int(self.reset_stop_flag_each_round_), _p(out),
                                                 _p(outl), C.byref(nv), C.byref(it)), "svgpu_pose_optimize")
        return nv.value, out, outl[:n].copy(), it.value

    def optimize_batch_flat(self, poses_cw, obs_off, pos_w, uvr, inv_sigma_sq, huber, intr, select=None, active=None):
        """Several problems over one frame observation in one device call (svgpu_pose_optimize_batch): problem p is the entries
        obs_off[p] .. obs_off[p + 1] of the per-entry arrays whose `select` byte is non-zero (None: all), skipped when active[p] == 0 or
        fewer than 5 are selected.  Returns (num_valid[P], pose[P, 12], outlier[total], lm_iterations[P])."""
        off = np.ascontiguousarray(obs_off, np.int32).reshape(-1)
        P = len(off) - 1
        pose = np.ascontiguousarray(poses_cw, np.float64).reshape(-1, 12)
        pw, uv = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3), np.ascontiguousarray(uvr, np.float32).reshape(-1, 3)
        w, hb = np.ascontiguousarray(inv_sigma_sq, np.float32).reshape(-1), np.ascontiguousarray(huber, np.float32).reshape(-1)
        K = np.ascontiguousarray(intr, np.float64).reshape(5)
        sel = None if select is None else np.ascontiguousarray(select, np.uint8).reshape(-1)
        act = None if active is None else np.ascontiguousarray(active, np.uint8).reshape(-1)
        n = len(pw)
        if (P < 0 or len(pose) != P or any(len(a) != n for a in (uv, w, hb)) or (sel is not None and len(sel) != n)
                or (act is not None and len(act) != P) or (P > 0 and off[-1] != n)):
            raise ValueError("optimize_batch_flat: array lengths disagree")
        out, outl = np.zeros((max(P, 1), 12)), np.zeros(max(n, 1), np.uint8)
        nv, it = np.zeros(max(P, 1), np.int32), np.zeros(max(P, 1), np.int32)
        self.ctx.check(lib().svgpu_pose_optimize_batch(self.ctx.handle, P, _p(off), _p(pose), _p(act), _p(pw), _p(uv), _p(w), _p(hb), _p(sel), _p(K),
                                                       self.num_trials_robust_, self.num_trials_, self.num_each_iter_,
                                                       int(self.reset_stop_flag_each_round_), _p(out), _p(outl), _p(nv), _p(it)),
                       "svgpu_pose_optimize_batch")
        return nv[:P].copy(), out[:P].copy(), outl[:n].copy(), it[:P].copy()

    def optimize_device(self, pose_cw, n: int, pos_w_dev, uvr_dev, inv_sigma_sq_dev, huber_dev, intr):
        """Same with the observation arrays already on the device (torch tensors or raw device addresses)."""
        pose = np.ascontiguousarray(pose_cw, np.float64).reshape(12)
        K = np.ascontiguousarray(intr, np.float64).reshape(5)
        out, outl = np.zeros(12), np.zeros(max(n, 1), np.uint8)
        nv, it = C.c_int(0), C.c_int(0)
        self.ctx.check(lib().svgpu_pose_optimize_device(self.ctx.handle, _p(pose), n, _p(pos_w_dev), _p(uvr_dev), _p(inv_sigma_sq_dev), _p(huber_dev), _p(K),
                                                        self.num_trials_robust_, self.num_trials_, self.num_each_iter_,
                                                        int(self.reset_stop_flag_each_round_), _p(out), _p(outl), C.byref(nv), C.byref(it)),
                       "svgpu_pose_optimize_device")
        return nv.value, out, outl[:n].copy(), it.value


# ------------------------------------------------------------------------------------------------ Sim3 pose graph (loop correction)
class _PoseGraphStats(C.Structure):
    _fields_ = [("lm_iterations", C.c_int32), ("lm_trials", C.c_int32), ("pcg_iterations", C.c_int32), ("pcg_capped", C.c_int32),
                ("stopped_by_gain", C.c_int32), ("num_free", C.c_int32), ("initial_chi2", C.c_double), ("final_chi2", C.c_double),
                ("lambda_final", C.c_double)]


class _PoseGraphOptions(C.Structure):
    _fields_ = [("solver", C.c_int32), ("reserved", C.c_int32 * 3)]


class _PoseGraphSolverStats(C.Structure):
    _fields_ = [("solver", C.c_int32), ("ordering", C.c_int32), ("envelope_blocks", C.c_int32), ("max_column_rows", C.c_int32),
                ("failed_solves", C.c_int32)]


PG_SOLVERS = {"pcg": 0, "envelope": 1}  # svgpu_pose_graph_solver


def pose_graph_optimize(ctx: Context, sim3, fixed, edge_v1, edge_v2, edge_sim3_21, fix_scale=False, max_iterations=50, gain_threshold=1e-3, solver="pcg"):
    """optimize::graph_optimizer::optimize over flat arrays (svgpu_pose_graph_optimize): sim3 N x 8 (qx qy qz qw tx ty tz s), fixed N,
    edges as two index arrays and E x 8 measurements Sim3_21.  Returns a dict: sim3 (N x 8), pose_cw (N x 3 x 4, [R | t / s]) and the
    stats lm_iterations, lm_trials, pcg_iterations, pcg_capped, stopped_by_gain, num_free, initial_chi2, final_chi2, lambda_final.
    solver="envelope" solves the damped systems by the block envelope Cholesky (svgpu_pose_graph_optimize_ex); the dict then also holds
    solver, ordering, envelope_blocks, max_column_rows and failed_solves ("pcg": solver 0 and zeros)."""
    if solver not in PG_SOLVERS:
        raise ValueError(f"pose_graph_optimize: unknown solver {solver!r}")
    s = np.ascontiguousarray(sim3, np.float64).reshape(-1, 8)
    f = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    e1, e2 = np.ascontiguousarray(edge_v1, np.int32).reshape(-1), np.ascontiguousarray(edge_v2, np.int32).reshape(-1)
    m = np.ascontiguousarray(edge_sim3_21, np.float64).reshape(-1, 8)
    if len(f) != len(s) or len(e2) != len(e1) or len(m) != len(e1):
        raise ValueError("pose_graph_optimize: array lengths disagree")
    out, pose, st, sst = np.zeros_like(s), np.zeros((len(s), 3, 4), np.float64), _PoseGraphStats(), _PoseGraphSolverStats()
    args = (ctx.handle, len(s), _p(s), _p(f), len(e1), _p(e1), _p(e2), _p(m), int(bool(fix_scale)), int(max_iterations), float(gain_threshold),
            _p(out), _p(pose), C.cast(C.pointer(st), C.c_void_p))
    if solver == "pcg":
        ctx.check(lib().svgpu_pose_graph_optimize(*args), "svgpu_pose_graph_optimize")
    else:
        opt = _PoseGraphOptions(PG_SOLVERS[solver], (C.c_int32 * 3)(0, 0, 0))
        ctx.check(lib().svgpu_pose_graph_optimize_ex(*args, C.cast(C.pointer(opt), C.c_void_p), C.cast(C.pointer(sst), C.c_void_p)), "svgpu_pose_graph_optimize_ex")
    res = {k: getattr(st, k) for k, _ in _PoseGraphStats._fields_}
    res.update({k: getattr(sst, k) for k, _ in _PoseGraphSolverStats._fields_})
    res.update(sim3=out, pose_cw=pose)
    return res


def envelope_selftest_solve(ctx: Context, pair_a, pair_b, diag_blocks, pair_blocks, rhs):
    """svgpu_selftest_pose_graph_envelope_solve: the envelope solver alone on the block-sparse symmetric system with 7x7 blocks
    {diag_blocks (n, 7, 7), block (pair_a[k], pair_b[k]) = pair_blocks[k] and its transpose} x = rhs (n, 7).  Returns (status, x (n, 7),
    dict of the solver stats); status 6 (SVGPU_ERR_NUMERIC) with failed_solves 1 when the system is not positive definite."""
    d = np.ascontiguousarray(diag_blocks, np.float64).reshape(-1, 49)
    a, b = np.ascontiguousarray(pair_a, np.int32).reshape(-1), np.ascontiguousarray(pair_b, np.int32).reshape(-1)
    blk = np.ascontiguousarray(pair_blocks, np.float64).reshape(-1, 49)
    r = np.ascontiguousarray(rhs, np.float64).reshape(-1)
    if len(b) != len(a) or len(blk) != len(a) or len(r) != 7 * len(d):
        raise ValueError("envelope_selftest_solve: array lengths disagree")
    x, sst = np.zeros((len(d), 7)), _PoseGraphSolverStats()
    status = lib().svgpu_selftest_pose_graph_envelope_solve(ctx.handle, len(d), len(a), _p(a) if len(a) else None, _p(b) if len(a) else None, _p(d),
                                                            _p(blk) if len(a) else None, _p(r), _p(x), C.cast(C.pointer(sst), C.c_void_p))
    return status, x, {k: getattr(sst, k) for k, _ in _PoseGraphSolverStats._fields_}


def correct_landmarks(ctx: Context, sim3_before, sim3_after, ref_vertex, pos_w):
    """Step 5 of graph_optimizer::optimize (svgpu_pose_graph_correct_landmarks): sim3_after[ref]^-1 .map(sim3_before[ref] .map(pos_w))."""
    a, b = np.ascontiguousarray(sim3_before, np.float64).reshape(-1, 8), np.ascontiguousarray(sim3_after, np.float64).reshape(-1, 8)
    r, p = np.ascontiguousarray(ref_vertex, np.int32).reshape(-1), np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    if len(a) != len(b) or len(r) != len(p):
        raise ValueError("correct_landmarks: array lengths disagree")
    out = np.zeros_like(p)
    ctx.check(lib().svgpu_pose_graph_correct_landmarks(ctx.handle, len(a), _p(a), _p(b), len(p), _p(r), _p(p), _p(out)), "svgpu_pose_graph_correct_landmarks")
    return out


# ------------------------------------------------------------------------------------------------ pairwise Sim3 (loop validation)
class _Camera(C.Structure):
    _fields_ = [("model", C.c_int32), ("pad_", C.c_int32), ("cols", C.c_double), ("rows", C.c_double), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 5), ("focal_x_baseline", C.c_double), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class _Sim3OptView(C.Structure):
    _fields_ = [("cam", _Camera), ("pose_cw", C.c_double * 12)]


class _Sim3OptStats(C.Structure):
    _fields_ = [("lm_iterations", C.c_int32 * 2), ("lm_trials", C.c_int32 * 2), ("early_return", C.c_int32), ("num_survivors", C.c_int32),
                ("first_chi2", C.c_double * 2), ("last_chi2", C.c_double * 2), ("lambda_final", C.c_double)]


def _sim3opt_view(cam: dict, pose_cw):
    v = _Sim3OptView()
    for k in ("model", "cols", "rows", "fx", "fy", "cx", "cy"):
        setattr(v.cam, k, cam.get(k, 0))
    v.pose_cw[:] = [float(x) for x in np.asarray(pose_cw, np.float64).reshape(12)]
    return v


def sim3_transform_optimize_batch(ctx: Context, view1, views2, match_off, obs1, obs2, inv_sigma_sq1, inv_sigma_sq2, pos_w_1, pos_w_2, sim3_12,
                                  chi_sq=10.0, fix_scale=False, num_iter=10):
    """optimize::transform_optimizer::optimize for several candidates at once (svgpu_sim3_transform_optimize_batch).  view1: one
    (camera dict, pose_cw) shared by all problems, or a list of them, one per problem; views2: a list of (camera dict, pose_cw); camera
    dict: model (svgpu_camera_model), fx fy cx cy, cols rows.  match_off: P + 1 offsets into the per-match arrays obs1 / obs2 (n x 2),
    inv_sigma_sq1 / 2 (n), pos_w_1 / 2 (n x 3).  sim3_12: P x 8.  Returns a dict: sim3 (P x 8), num_inliers (P), status (n) and the
    per-problem stats lm_iterations, lm_trials, first_chi2, last_chi2 (P x 2 each), early_return, num_survivors, lambda_final (P)."""
    off = np.ascontiguousarray(match_off, np.int32).reshape(-1)
    P = len(off) - 1
    shared = isinstance(view1, tuple)
    v1 = [view1] if shared else list(view1)
    if P < 0 or len(views2) != P or (not shared and len(v1) != P):
        raise ValueError("sim3_transform_optimize_batch: array lengths disagree")
    V1 = (_Sim3OptView * max(len(v1), 1))(*[_sim3opt_view(c, p) for c, p in v1])
    V2 = (_Sim3OptView * max(P, 1))(*[_sim3opt_view(c, p) for c, p in views2])
    o1, o2 = np.ascontiguousarray(obs1, np.float64).reshape(-1, 2), np.ascontiguousarray(obs2, np.float64).reshape(-1, 2)
    w1, w2 = np.ascontiguousarray(inv_sigma_sq1, np.float32).reshape(-1), np.ascontiguousarray(inv_sigma_sq2, np.float32).reshape(-1)
    p1, p2 = np.ascontiguousarray(pos_w_1, np.float64).reshape(-1, 3), np.ascontiguousarray(pos_w_2, np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(sim3_12, np.float64).reshape(-1, 8)
    n = len(o1)
    if len(s) != P or any(len(a) != n for a in (o2, w1, w2, p1, p2)) or (P > 0 and off[-1] != n):
        raise ValueError("sim3_transform_optimize_batch: array lengths disagree")
    out, inl, status = np.zeros_like(s), np.zeros(max(P, 1), np.int32), np.zeros(max(n, 1), np.uint8)
    st = (_Sim3OptStats * max(P, 1))()
    ctx.check(lib().svgpu_sim3_transform_optimize_batch(ctx.handle, P, C.cast(V1, C.c_void_p), int(shared), C.cast(V2, C.c_void_p), _p(off), _p(o1), _p(o2),
                                                        _p(w1), _p(w2), _p(p1), _p(p2), _p(s), chi_sq, int(bool(fix_scale)), int(num_iter),
                                                        _p(out), _p(inl), _p(status), C.cast(st, C.c_void_p)), "svgpu_sim3_transform_optimize_batch")
    res = dict(sim3=out, num_inliers=inl[:P].copy(), status=status[:n].copy())
    for k, _ in _Sim3OptStats._fields_:
        res[k] = np.array([np.array(getattr(st[p], k)) for p in range(P)])
    return res


def sim3_transform_optimize(ctx: Context, view1, view2, obs1, obs2, inv_sigma_sq1, inv_sigma_sq2, pos_w_1, pos_w_2, sim3_12, chi_sq=10.0,
                            fix_scale=False, num_iter=10):
    """One candidate (svgpu_sim3_transform_optimize): view1 / view2 are (camera dict, pose_cw).  Returns the dict of the batch call with
    the problem axis dropped."""
    o1, o2 = np.ascontiguousarray(obs1, np.float64).reshape(-1, 2), np.ascontiguousarray(obs2, np.float64).reshape(-1, 2)
    w1, w2 = np.ascontiguousarray(inv_sigma_sq1, np.float32).reshape(-1), np.ascontiguousarray(inv_sigma_sq2, np.float32).reshape(-1)
    p1, p2 = np.ascontiguousarray(pos_w_1, np.float64).reshape(-1, 3), np.ascontiguousarray(pos_w_2, np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(sim3_12, np.float64).reshape(8)
    n = len(o1)
    if any(len(a) != n for a in (o2, w1, w2, p1, p2)):
        raise ValueError("sim3_transform_optimize: array lengths disagree")
    V1, V2 = _sim3opt_view(*view1), _sim3opt_view(*view2)
    out, inl, status, st = np.zeros(8), C.c_int32(0), np.zeros(max(n, 1), np.uint8), _Sim3OptStats()
    ctx.check(lib().svgpu_sim3_transform_optimize(ctx.handle, C.byref(V1), C.byref(V2), n, _p(o1), _p(o2), _p(w1), _p(w2), _p(p1), _p(p2), _p(s),
                                                  chi_sq, int(bool(fix_scale)), int(num_iter), _p(out), C.byref(inl), _p(status), C.byref(st)),
              "svgpu_sim3_transform_optimize")
    res = dict(sim3=out, num_inliers=int(inl.value), status=status[:n].copy())
    for k, _ in _Sim3OptStats._fields_:
        v = getattr(st, k)
        res[k] = np.array(v) if hasattr(v, "__len__") else v
    return res
