"""Numpy restatement of svgpu_sim3_transform_optimize (optimize::transform_optimizer::optimize, optimize/transform_optimizer.cc:20-158) and
the planted problem classes of its tests.

The restatement is written once over a dtype and used in two forms:
  fp64          np.float64, the damped 7x7 system solved by LAPACK (np.linalg.solve)
  long double   np.longdouble, the damped system factored by a hand-written Cholesky
Both follow g2o as the device does.  One 7-dof vertex Sim3_12 (the Sim3 functions of tests/posegraph_problems.py) and two unary edges per
match:
  forward    e12 = obs1 - project1(S12.map(R_2w pos_w_2 + t_2w))         internal/sim3/forward_reproj_edge.h:61-76
  backward   e21 = obs2 - project2(S12^-1.map(R_1w pos_w_1 + t_1w))      internal/sim3/backward_reproj_edge.h:61-77
information = inv_sigma_sq (a float) times identity, chi2 = info |e|^2, Huber of width sqrtf(chi_sq) on every edge in both stages with
first-order weighting, Jacobians by central differences (delta 1e-9) through exp(update) * estimate (coordinate 6 of the update zeroed
under fix_scale), Levenberg-Marquardt exactly as tests/posegraph_problems.py `optimize` states it but without terminate_action, restarted
per stage.  Stage 1: 5 iterations over all edges, then `chi2_12 < chi_sq && chi2_21 < chi_sq` keeps a match; fewer than 10 survivors:
0 inliers and the input Sim3.  Stage 2: num_iter iterations over the survivors, then `chi_sq < chi2_12 || chi_sq < chi2_21` rejects.  The
chi2 a gate reads is the edge's cached error: that of the stage's last evaluation, i.e. its last damping trial, accepted or not.

A problem is a dict: cam1 / cam2 (dicts: model, fx, fy, cx, cy, cols, rows), pose1 / pose2 (12,) rows of [R | t] world -> camera,
obs1 / obs2 (n, 2), w1 / w2 (n,) float32, pos1 / pos2 (n, 3) landmarks of keyframe 1 / 2 in their worlds, sim3 (8,), chi_sq float32,
fix_scale bool, num_iter int.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import posegraph_problems as G

DELTA = 1e-9
PERSPECTIVE, FISHEYE, EQUIRECTANGULAR, RADIAL_DIVISION = 0, 1, 2, 3
STAGE1_ITER = 5
MIN_SURVIVORS = 10
deviation = G.deviation


# ------------------------------------------------------------------------------------------------------------------ edges
def project(cam, p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    t = p.dtype.type
    if cam["model"] == EQUIRECTANGULAR:
        pi = t(np.pi)
        theta = np.arctan2(x, z)
        phi = -np.arcsin(y / np.sqrt(x * x + y * y + z * z))
        return np.stack([t(cam["cols"]) * (t(0.5) + theta / (2 * pi)), t(cam["rows"]) * (t(0.5) - phi / pi)], -1)
    return np.stack([t(cam["fx"]) * x / z + t(cam["cx"]), t(cam["fy"]) * y / z + t(cam["cy"])], -1)


def _cam_points(pose, pos, dtype):
    T = np.asarray(pose, dtype).reshape(3, 4)
    X = np.asarray(pos, dtype)
    return np.stack([T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1] + T[r, 2] * X[:, 2] + T[r, 3] for r in range(3)], -1)


class _Edges:
    """The 2 n edges of a problem in the order they are added: match i gives edge 2 i (forward) and 2 i + 1 (backward)."""

    def __init__(self, prob, dtype):
        self.n = n = len(prob["obs1"])
        self.dtype = dtype
        self.cam1, self.cam2 = prob["cam1"], prob["cam2"]
        self.p2c = _cam_points(prob["pose2"], prob["pos2"], dtype)  # R_2w pos_w_2 + t_2w
        self.p1c = _cam_points(prob["pose1"], prob["pos1"], dtype)
        self.obs1, self.obs2 = np.asarray(prob["obs1"], dtype).reshape(n, 2), np.asarray(prob["obs2"], dtype).reshape(n, 2)
        w = np.empty(2 * n, dtype)
        w[0::2] = np.asarray(prob["w1"], np.float32).astype(dtype)
        w[1::2] = np.asarray(prob["w2"], np.float32).astype(dtype)
        self.w = w

    def errors(self, S):
        """(..., 2 n, 2) for Sim3s of shape (..., 8)"""
        Sf, Si = S[..., None, :], G.sim3_inv(S)[..., None, :]
        e12 = self.obs1 - project(self.cam1, G.sim3_map(Sf, self.p2c))
        e21 = self.obs2 - project(self.cam2, G.sim3_map(Si, self.p1c))
        out = np.empty(e12.shape[:-2] + (2 * self.n, 2), self.dtype)
        out[..., 0::2, :] = e12
        out[..., 1::2, :] = e21
        return out

    def chi2(self, e):
        return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) * self.w


def huber(chi, delta):
    """g2o's RobustKernelHuber as oracle/ba_oracle.c states it: rho0, rho1"""
    dsqr = delta * delta
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(chi)
        inl = chi <= dsqr
        return np.where(inl, chi, 2 * sq * delta - dsqr), np.where(inl, chi.dtype.type(1), delta / np.where(inl, 1, sq))


def cholesky_solve(A, b):
    """Unrolled LL^T of the damped 7x7 system as the device factors it; None when a pivot is not positive."""
    n = len(b)
    L = A.copy()
    for j in range(n):
        d = L[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            return None
        d = np.sqrt(d)
        L[j, j] = d
        for i in range(j + 1, n):
            L[i, j] = (L[i, j] - (L[i, :j] * L[j, :j]).sum()) / d
    x = np.zeros(n, A.dtype)
    for i in range(n):
        x[i] = (b[i] - (L[i, :i] * x[:i]).sum()) / L[i, i]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


# ------------------------------------------------------------------------------------------------------------------ the optimizer
def optimize(prob, dtype=np.float64, num_iter=None):
    """The whole call.  Returns sim3, num_inliers, status (n,), early_return, lm_iterations / lm_trials / first_chi2 / last_chi2 (two
    entries each, one per stage), lambda_final, and what the decision filter looks at: `seq` (stage, iteration, accepted) per trial,
    `rhos` per trial and `gate_chi2`, every chi2 a gate read."""
    dtype = np.dtype(dtype).type
    num_iter = int(prob["num_iter"]) if num_iter is None else int(num_iter)
    E = _Edges(prob, dtype)
    n = E.n
    chi_sq = dtype(np.float32(prob["chi_sq"]))
    delta = dtype(np.sqrt(np.float32(prob["chi_sq"])))  # (double)sqrtf(chi_sq)
    S0 = np.asarray(prob["sim3"], np.float64).reshape(8)
    S = S0.astype(dtype)
    U = np.zeros((7, 2, 7), dtype)
    for c in range(7):
        if prob["fix_scale"] and c == 6:
            continue
        U[c, 0, c], U[c, 1, c] = DELTA, -DELTA
    X = G.sim3_exp(U)  # (7, 2, 8)
    scalar = dtype(1) / (2 * dtype(DELTA))
    out = dict(lm_iterations=[0, 0], lm_trials=[0, 0], first_chi2=[0.0, 0.0], last_chi2=[0.0, 0.0], lambda_final=0.0, seq=[], rhos=[], gate_chi2=[],
               early_return=0)
    status = np.zeros(n, np.uint8)
    cache = np.zeros(2 * n, dtype)  # g2o's cached _error of every edge, as its chi2
    lam = dtype(0)

    def robust_sum(chi, act):
        return huber(chi, delta)[0][act].sum()

    for stage in range(2):
        iters = STAGE1_ITER if stage == 0 else num_iter
        act = np.repeat(status == 0, 2)
        ok, ni = True, dtype(2)
        it = 0
        while it < iters and ok and n > 0:
            e0 = E.errors(S)
            ep = E.errors(G.sim3_mul(X, S))                # (7, 2, 2 n, 2)
            J = scalar * (ep[:, 0] - ep[:, 1])             # (7, 2 n, 2): [column, edge, row]
            chi = E.chi2(e0)
            rho0, rho1 = huber(chi, delta)
            wt = np.where(act, E.w * rho1, 0)
            H = np.einsum("aer,e,cer->ac", J, wt, J)
            b = np.einsum("aer,er->a", J, -wt[:, None] * e0)
            current = rho0[act].sum()
            if it == 0:
                lam, ni = dtype(1e-5) * np.abs(np.diag(H)).max(), dtype(2)
                out["first_chi2"][stage] = float(current)
            rho, qmax = dtype(0), 0
            while True:
                A = H + lam * np.eye(7, dtype=dtype)
                if dtype is np.float64:
                    try:
                        np.linalg.cholesky(A)
                        dx = np.linalg.solve(A, b)
                    except np.linalg.LinAlgError:
                        dx = None
                else:
                    dx = cholesky_solve(A, b)
                solved = dx is not None
                if not solved:
                    dx = np.zeros(7, dtype)
                u = dx.copy()
                if prob["fix_scale"]:
                    u[6] = 0
                trial = G.sim3_mul(G.sim3_exp(u), S)
                chit = E.chi2(E.errors(trial))
                cache = np.where(act, chit, cache)
                temp = robust_sum(chit, act) if solved else dtype(np.finfo(np.float64).max)
                scale = (dx * (lam * dx + b)).sum() + dtype(1e-3)
                rho = (current - temp) / scale
                accepted = bool(rho > 0 and np.isfinite(temp))
                out["lm_trials"][stage] += 1
                out["seq"].append((stage, it, accepted))
                out["rhos"].append(float(rho))
                if accepted:
                    alpha = min(1 - (2 * rho - 1) ** 3, dtype(2) / 3)
                    lam = lam * max(dtype(1) / 3, alpha)
                    ni = dtype(2)
                    current = temp
                    S = trial
                else:
                    lam = lam * ni
                    ni = ni * 2
                    if not np.isfinite(lam):
                        break
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0 or not np.isfinite(lam):
                ok = False
            out["last_chi2"][stage] = float(current)
            it += 1
        out["lm_iterations"][stage] = it
        c12, c21 = cache[0::2], cache[1::2]
        live = status == 0
        out["gate_chi2"] += [float(v) for v in np.stack([c12, c21], -1)[live].ravel()]
        if stage == 0:
            status[~((c12 < chi_sq) & (c21 < chi_sq))] = 1
            out["survivors"] = int((status == 0).sum())
            if out["survivors"] < MIN_SURVIVORS:
                out["early_return"] = 1
                break
        else:
            status[live & ((chi_sq < c12) | (chi_sq < c21))] = 2
    out["lambda_final"] = float(lam)
    out["status"] = status
    out["num_inliers"] = 0 if out["early_return"] else int((status == 0).sum())
    out["sim3"] = S0.astype(dtype) if out["early_return"] else S
    return out


# ------------------------------------------------------------------------------------------------------------------ planted problems
def pinhole(fx=520.0, fy=515.0, cx=320.5, cy=240.25, model=PERSPECTIVE):
    return dict(model=model, fx=fx, fy=fy, cx=cx, cy=cy, cols=640.0, rows=480.0)


def equirect(cols=1920.0, rows=960.0):
    return dict(model=EQUIRECTANGULAR, fx=0.0, fy=0.0, cx=0.0, cy=0.0, cols=cols, rows=rows)


def _pose(rotvec, t):
    q = G.make_sim3(np.asarray(rotvec, float), np.zeros(3), 1.0)[:4]
    return np.concatenate([G.quat_to_rot(q), np.asarray(t, float)[:, None]], 1).reshape(12)


def _pose_inv_map(pose, pc):
    T = pose.reshape(3, 4)
    return (pc - T[:, 3]) @ T[:, :3]


def _scene(seed, n, cam1, cam2, fix_scale, num_iter, true_scale=1.0, noise_px=0.5, gross=0, octaves=(0,), all_sides=False, depth=(500.0, 1200.0),
           chi_sq=10.0):
    """n physical points seen by both keyframes.  Keyframe 2 lives in a drifted world: Sim3_12 (camera 2 -> camera 1) has the scale
    `true_scale`.  The last `gross` matches are gross mismatches (keyframe 2's keypoint is somewhere else).  The start is off the truth by
    about 2 degrees, 0.05 and (unless the scale is fixed) 3 %.

    The points are far away next to that translation (depth 500 .. 1200).  With points a few units away Levenberg-Marquardt is at the
    rounding floor of chi2 after four iterations, and from then on every gain ratio rho is rounding noise around zero (measured: 1e-9 and
    below from stage 1's fifth iteration on, with either sign): which trials are accepted is then an accident of the implementation, and
    no seed changes that.  With a weakly observed translation the damping term governs the step along it, chi2 keeps falling by a
    macroscopic amount through all of stage 1 and stage 2, and every rho stays of order 0.1 .. 1 in both forms."""
    rng = np.random.default_rng(seed)
    if all_sides:
        d = rng.normal(size=(n, 3))
        d[:, 2] = np.abs(d[:, 2]) * np.where(np.arange(n) % 2, -1.0, 1.0)  # every other point behind the camera: z < 0
        P1 = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(depth[0], depth[1], size=(n, 1))
    else:
        P1 = np.stack([rng.uniform(-0.45, 0.45, n), rng.uniform(-0.35, 0.35, n), np.ones(n)], -1) * rng.uniform(depth[0], depth[1], size=(n, 1))
    true = G.make_sim3(np.array([0.03, -0.12, 0.02]), np.array([0.4, -0.05, 0.1]), true_scale)
    P2 = G.sim3_map(G.sim3_inv(true), P1)
    pose1 = _pose([0.2, -0.4, 0.1], [0.3, -1.0, 2.0])
    pose2 = _pose([-0.1, 0.7, 0.05], [-1.5, 0.2, 0.7])
    oct1, oct2 = rng.choice(octaves, n), rng.choice(octaves, n)
    inv_sigma_sq = lambda o: np.float32(1.0) / (np.float32(1.2) ** o.astype(np.float32)) ** 2
    obs1 = project(cam1, P1) + rng.normal(size=(n, 2)) * noise_px * (1.2 ** oct1)[:, None]
    obs2 = project(cam2, P2) + rng.normal(size=(n, 2)) * noise_px * (1.2 ** oct2)[:, None]
    if gross:
        sign = np.where(rng.random((gross, 2)) < 0.5, -1.0, 1.0)
        obs2[n - gross:] += sign * rng.uniform(25.0, 60.0, size=(gross, 2))
    axis = rng.normal(size=3)
    off = G.make_sim3(axis / np.linalg.norm(axis) * np.deg2rad(2.0), rng.normal(size=3) / np.sqrt(3.0) * 0.05, 1.0 if fix_scale else 1.03)
    start = G.sim3_mul(off, true)
    start[:4] /= np.sqrt((start[:4] ** 2).sum())
    return dict(cam1=cam1, cam2=cam2, pose1=pose1, pose2=pose2, obs1=np.ascontiguousarray(obs1), obs2=np.ascontiguousarray(obs2),
                w1=inv_sigma_sq(oct1).astype(np.float32), w2=inv_sigma_sq(oct2).astype(np.float32), pos1=_pose_inv_map(pose1, P1),
                pos2=_pose_inv_map(pose2, P2), sim3=start, chi_sq=np.float32(chi_sq), fix_scale=bool(fix_scale), num_iter=int(num_iter), true=true,
                p1c_z=P1[:, 2].copy())


WORKGROUP_EDGES = 256  # threads of the device's workgroup: one edge each, i.e. 128 matches per pass; a wavefront holds 32 matches
SIZES = (10, 31, 32, 33, 127, 128, 129, 255, 256, 257)

# class -> keyword arguments of _scene.  The seed, the depth range and stage 2's iteration count below are fixed so that EVERY case passes
# the decision filter of tests/test_sim3opt_problem_classes.py in both forms (no case is skipped or re-drawn at run time)
_CLASSES = {}


def _add(name, fs_values=(0, 1), **kw):
    for fs in fs_values:
        _CLASSES[f"{name}-fs{fs}"] = dict(kw, fix_scale=fs)


_add("a", n=40, cam1=pinhole(), cam2=pinhole(480.0, 482.0, 330.0, 250.0))
_add("b", n=40, gross=10, cam1=pinhole(), cam2=pinhole(480.0, 482.0, 330.0, 250.0))
_add("c", n=48, cam1=equirect(), cam2=equirect(), all_sides=True)
_add("d", n=40, cam1=pinhole(model=RADIAL_DIVISION), cam2=equirect(), octaves=(0, 1, 2, 3))
_add("e0.5", n=40, cam1=pinhole(), cam2=pinhole(model=FISHEYE), true_scale=0.5)
_add("e2", n=40, cam1=pinhole(), cam2=pinhole(), true_scale=2.0)
_add("f12", n=12, gross=3, cam1=pinhole(), cam2=pinhole())
_add("f13", n=13, gross=3, cam1=pinhole(), cam2=pinhole())
for _n in SIZES:
    _add(f"g{_n}", fs_values=(_n % 2,), n=_n, gross=_n // 8 if _n > 10 else 0, cam1=pinhole(), cam2=pinhole())

SEED, NUM_ITER = 1, 4
CASES = list(_CLASSES)


def problem(case):
    return _scene(SEED, num_iter=NUM_ITER, **_CLASSES[case])


@functools.lru_cache(maxsize=None)
def solved(case, form):
    """The restatement's result on a case, computed once per process and shared (treat it as read-only)."""
    return optimize(problem(case), np.float64 if form == "fp64" else np.longdouble)


def two_form_deviation(case):
    return deviation(solved(case, "fp64")["sim3"][None], solved(case, "ld")["sim3"][None])


@functools.lru_cache(maxsize=None)
def common_floor():
    """F: the median two-form deviation over all cases"""
    return float(np.median([two_form_deviation(c) for c in CASES]))


def bound(case):
    return 16.0 * max(two_form_deviation(case), common_floor())


def filter_margins(res, chi_sq):
    """(smallest relative distance of a gate chi2 from chi_sq, smallest |rho|) of one result"""
    g = np.asarray(res["gate_chi2"], np.float64)
    gate = float(np.abs(g - float(chi_sq)).min() / float(chi_sq)) if len(g) else np.inf
    rho = float(np.abs(res["rhos"]).min()) if res["rhos"] else np.inf
    return gate, rho
