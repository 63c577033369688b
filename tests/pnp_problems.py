"""Problems and the CPU yardstick for the PnP solver (svgpu_pnp_compute_pose, svgpu_pnp_ransac[_batch]).

The yardstick is a restatement of solve::pnp_solver (solve/pnp_solver.cc) in numpy: fp64 arithmetic in the reference's operation order,
np.float32 where the reference has `float` (max_cos_errors_), the decompositions from LAPACK (np.linalg.svd).  With dtype = np.longdouble
the same steps run in extended precision and every decomposition comes from a Jacobi iteration in that precision: that result calibrates
the tolerances.  `null_rot` rotates the four singular vectors EPnP uses inside their span: for a four-point sample they span the whole
null space of M^T M, every orthonormal basis of it is as good as Eigen's, and what a hypothesis gives depends on the choice.
`check_inliers` also returns, per match, the relative distance of cos_angle from its threshold (the "margin").
numpy only; shared by tests/test_pnp_problem_classes.py (CPU) and tests/test_gpu_pnp.py (GPU)."""
import numpy as np

F32 = np.float32
DBL_MAX = np.finfo(np.float64).max
MATCH_COUNTS = (4, 5, 63, 64, 65, 300)
OVERDETERMINED = (6, 7, 63, 64, 65, 300)


def orb_scale_factors(scale_factor=1.2, num_levels=8):
    """feature/orb_params.cc: fp32 recurrence."""
    sf = np.ones(num_levels, F32)
    for l in range(1, num_levels):
        sf[l] = F32(scale_factor) * sf[l - 1]
    return sf


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


# ------------------------------------------------------------------------------------------------ util::cos, max_cos_errors_
def _cos_poly(v):
    c1, c2, c3 = F32(0.99940307), F32(-0.49558072), F32(0.03679168)
    v2 = F32(v * v)
    return F32(c1 + F32(v2 * F32(c2 + F32(c3 * v2))))


def util_cos(v):
    """util/trigonometric.h:26-42, float."""
    PI = F32(3.14159265358979)
    PI_2, TWO_PI = F32(PI / F32(2.0)), F32(F32(2.0) * PI)
    INV_TWO_PI, THREE_PI_2 = F32(F32(1.0) / TWO_PI), F32(F32(3.0) * PI_2)
    v = F32(v)
    v = F32(v - F32(F32(int(np.floor(F32(v * INV_TWO_PI)))) * TWO_PI))
    v = v if F32(0.0) < v else F32(-v)
    if v < PI_2:
        return _cos_poly(v)
    if v < PI:
        return F32(-_cos_poly(F32(PI - v)))
    if v < THREE_PI_2:
        return F32(-_cos_poly(F32(v - PI)))
    return _cos_poly(F32(TWO_PI - v))


def max_cos_errors(octaves, scale_factors):
    """pnp_solver.cc:27-32: util::cos(scale_factors.at(octave) * (1.0 * M_PI / 180.0)); the product is a double, the argument a float."""
    sf = np.asarray(scale_factors, F32)
    table = np.array([util_cos(F32(float(s) * (1.0 * np.pi / 180.0))) for s in sf], F32)
    return table[np.asarray(octaves, np.int64)]


# ------------------------------------------------------------------------------------------------ decompositions
def jacobi_sym(A, dtype=np.longdouble, sweeps=60):
    """Cyclic Jacobi of a symmetric matrix in `dtype`: eigenvalues in descending order and their eigenvectors (columns)."""
    a = np.array(A, dtype=dtype)
    n = len(a)
    v = np.eye(n, dtype=dtype)
    eps = np.finfo(dtype).eps
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = a[p, q]
                    if apq == 0 or not abs(apq) > eps * np.sqrt(abs(a[p, p] * a[q, q])):
                        continue
                    rotated = True
                    theta = (a[q, q] - a[p, p]) / (2 * apq)
                    t = np.copysign(dtype(1), theta) / (abs(theta) + np.sqrt(1 + theta * theta))
                    c = 1 / np.sqrt(1 + t * t)
                    s = c * t
                    G = np.eye(n, dtype=dtype)
                    G[p, p] = G[q, q] = c
                    G[p, q], G[q, p] = s, -s
                    a = G.T @ a @ G
                    a[p, q] = a[q, p] = 0
                    v = v @ G
            if not rotated:
                break
    d = np.diag(a).copy()
    order = np.argsort(-d, kind="stable")
    return d[order], v[:, order]


def jacobi_svd(A, dtype=np.longdouble, sweeps=60):
    """One-sided (Hestenes) Jacobi in `dtype`: thin U (m x k, a zero column where the singular value is zero), s descending, V (k x k)."""
    a = np.array(A, dtype=dtype)
    m, k = a.shape
    v = np.eye(k, dtype=dtype)
    eps = np.finfo(dtype).eps
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            rotated = False
            for p in range(k - 1):
                for q in range(p + 1, k):
                    al, be, ga = a[:, p] @ a[:, p], a[:, q] @ a[:, q], a[:, p] @ a[:, q]
                    if ga == 0 or not abs(ga) > eps * np.sqrt(al * be):
                        continue
                    rotated = True
                    zeta = (be - al) / (2 * ga)
                    t = np.copysign(dtype(1), zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = 1 / np.sqrt(1 + t * t)
                    s = c * t
                    ap, aq, vp, vq = a[:, p].copy(), a[:, q].copy(), v[:, p].copy(), v[:, q].copy()
                    a[:, p], a[:, q] = c * ap - s * aq, s * ap + c * aq
                    v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
            if not rotated:
                break
        sv = np.sqrt((a * a).sum(0))
        order = np.argsort(-sv, kind="stable")
        sv, a, v = sv[order], a[:, order], v[:, order]
        u = np.where(sv > 0, a / np.where(sv > 0, sv, 1), 0)
    return u, sv, v


def _sym_usv(A, dtype, jacobi=False):
    """U and singular values of a symmetric positive semi-definite matrix (JacobiSVD of PW0^T PW0 and of M^T M)."""
    if dtype == np.float64 and not jacobi:
        u, s, _ = np.linalg.svd(A)
        return u, s
    d, v = jacobi_sym(A, dtype)
    return v, np.maximum(d, 0)


def _svd(A, dtype, jacobi=False):
    """thin U, s, V of a general matrix."""
    if dtype == np.float64 and not jacobi:
        u, s, vt = np.linalg.svd(A, full_matrices=False)
        return u, s, vt.T
    return jacobi_svd(A, dtype)


def _svd_solve(A, rhs, dtype, jacobi=False):
    """JacobiSVD::solve with Eigen's rank rule (SVDBase::rank: s_j >= max(s_0 * diagSize * epsilon, DBL_MIN); the rule is fp64's in either precision)."""
    u, s, v = _svd(A, dtype, jacobi)
    keep = max(s[0] * (min(A.shape) * np.finfo(np.float64).eps), np.finfo(np.float64).tiny)
    r = int((~(s < keep)).sum())
    return v[:, :r] @ ((u[:, :r].T @ rhs) / s[:r])


def _householder_solve(A, b):
    """A.householderQr().solve(b) as Eigen's unblocked kernel forms it, in the dtype of A."""
    a = np.concatenate([A, b[:, None]], 1).copy()
    rows, cols = A.shape
    tiny = np.finfo(np.float64).tiny
    with np.errstate(all="ignore"):
        for k in range(cols):
            tail = (a[k + 1:, k] * a[k + 1:, k]).sum()
            c0 = a[k, k]
            if tail <= tiny:
                tau, beta = 0, c0
                a[k + 1:, k] = 0
            else:
                beta = np.sqrt(c0 * c0 + tail)
                if c0 >= 0:
                    beta = -beta
                a[k + 1:, k] = a[k + 1:, k] / (c0 - beta)
                tau = (beta - c0) / beta
            a[k, k] = beta
            ess = a[k + 1:, k]
            for c in range(k + 1, cols + 1):
                tmp = ess @ a[k + 1:, c] + a[k, c]
                a[k, c] -= tau * tmp
                a[k + 1:, c] -= tau * ess * tmp
        x = a[:cols, cols].copy()
        for i in range(cols - 1, -1, -1):
            x[i] = x[i] / a[i, i]
            x[:i] -= a[:i, i] * x[i]
    return x


# ------------------------------------------------------------------------------------------------ compute_pose
_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
_L_COLS = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3))


def _initial_betas(L, rho, N, dtype, jacobi=False):
    bt = np.zeros(4, dtype)
    with np.errstate(all="ignore"):
        if N == 4:
            b = _svd_solve(L[:, [0, 1, 3, 6]], rho, dtype, jacobi)
            if b[0] < 0:
                bt[0] = np.sqrt(-b[0])
                bt[1:] = -b[1:] / bt[0]
            else:
                bt[0] = np.sqrt(b[0])
                bt[1:] = b[1:] / bt[0]
            return bt
        b = _svd_solve(L[:, :3] if N == 2 else L[:, :5], rho, dtype, jacobi)
        if b[0] < 0:
            bt[0] = np.sqrt(-b[0])
            bt[1] = np.sqrt(-b[2]) if b[2] < 0 else 0
        else:
            bt[0] = np.sqrt(b[0])
            bt[1] = np.sqrt(b[2]) if b[2] > 0 else 0
        if b[1] < 0:
            bt[0] = -bt[0]
        if N == 3:
            bt[2] = b[3] / bt[0]
    return bt


def _gauss_newton(L, rho, bt, num_iter):
    bt = bt.copy()
    with np.errstate(all="ignore"):
        for _ in range(num_iter):
            A = np.empty((6, 4), bt.dtype)
            A[:, 0] = 2 * L[:, 0] * bt[0] + L[:, 1] * bt[1] + L[:, 3] * bt[2] + L[:, 6] * bt[3]
            A[:, 1] = L[:, 1] * bt[0] + 2 * L[:, 2] * bt[1] + L[:, 4] * bt[2] + L[:, 7] * bt[3]
            A[:, 2] = L[:, 3] * bt[0] + L[:, 4] * bt[1] + 2 * L[:, 5] * bt[2] + L[:, 8] * bt[3]
            A[:, 3] = L[:, 6] * bt[0] + L[:, 7] * bt[1] + L[:, 8] * bt[2] + 2 * L[:, 9] * bt[3]
            b = rho - (L[:, 0] * bt[0] * bt[0] + L[:, 1] * bt[0] * bt[1] + L[:, 2] * bt[1] * bt[1] + L[:, 3] * bt[0] * bt[2] + L[:, 4] * bt[1] * bt[2]
                       + L[:, 5] * bt[2] * bt[2] + L[:, 6] * bt[0] * bt[3] + L[:, 7] * bt[1] * bt[3] + L[:, 8] * bt[2] * bt[3] + L[:, 9] * bt[3] * bt[3])
            bt = bt + _householder_solve(A, b)
    return bt


def _cos_angles(R, t, brg, pw):
    """pos_c = rot * pos_w + trans and pos_c.dot(bearing) / pos_c.norm(), elementwise and left to right (no matrix product: a BLAS may fuse)."""
    x, y, z = pw[:, 0], pw[:, 1], pw[:, 2]
    X = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
    Y = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
    Z = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
    return ((X * brg[:, 0] + Y * brg[:, 1]) + Z * brg[:, 2]) / np.sqrt((X * X + Y * Y) + Z * Z)


def reprojection_error(R, t, brg, pw):
    with np.errstate(all="ignore"):
        return (1.0 - _cos_angles(R, t, brg, pw)).sum() / len(pw)


def compute_pose(bearings, pos_w, gn_iter=10, dtype=np.float64, null_rot=None, jacobi=False):
    """pnp_solver::compute_pose (:155-206).  Returns R, t, reproj_error (fp64; NaN pose when no N gave a comparable error) and the twelve
    singular values of M^T M.  jacobi: in fp64 too every decomposition comes from the Jacobi iterations (signs and order as in long double)."""
    brg, pw = np.asarray(bearings, np.float64).astype(dtype), np.asarray(pos_w, np.float64).astype(dtype)
    n = len(pw)
    with np.errstate(all="ignore"):
        c0 = pw.sum(0) / n
        PW0 = pw - c0
        U3, D3 = _sym_usv(PW0.T @ PW0, dtype, jacobi)
        cws = np.stack([c0] + [c0 + np.sqrt(D3[i] / n) * U3[:, i] for i in range(3)])
        CC = (cws[1:] - cws[0]).T
        u, D, v = _svd(CC, dtype, jacobi)
        S = np.array([1 / d if d > 1e-6 else 0 for d in D], dtype)
        CC_inv = (v * S) @ u.T
        alphas = np.empty((n, 4), dtype)
        alphas[:, 1:] = (pw - cws[0]) @ CC_inv.T
        alphas[:, 0] = 1.0 - alphas[:, 1] - alphas[:, 2] - alphas[:, 3]
        uu, vv = brg[:, 0] / brg[:, 2], brg[:, 1] / brg[:, 2]
        M = np.zeros((2 * n, 12), dtype)
        for i in range(4):
            M[0::2, 3 * i] = alphas[:, i]
            M[0::2, 3 * i + 2] = -alphas[:, i] * uu
            M[1::2, 3 * i + 1] = alphas[:, i]
            M[1::2, 3 * i + 2] = -alphas[:, i] * vv
        U, sv = _sym_usv(M.T @ M, dtype, jacobi)
        Un = U[:, [11, 10, 9, 8]]  # Un[:, j] = U.col(11 - j)
        if null_rot is not None:
            Un = Un @ np.asarray(null_rot, np.float64).astype(dtype)
        dv = np.stack([[Un[3 * a:3 * a + 3, x] - Un[3 * b:3 * b + 3, x] for a, b in _PAIRS] for x in range(4)])  # dv[x, i]
        L = np.empty((6, 10), dtype)
        for c, (x, y) in enumerate(_L_COLS):
            d = (dv[x] * dv[y]).sum(1)
            L[:, c] = d if x == y else 2 * d
        rho = np.array([((cws[a] - cws[b]) ** 2).sum() for a, b in _PAIRS], dtype)
        best, R_best, t_best = DBL_MAX, np.full((3, 3), np.nan), np.full(3, np.nan)
        for N in (2, 3, 4):
            bt = _gauss_newton(L, rho, _initial_betas(L, rho, N, dtype, jacobi), gn_iter)
            ccs = np.stack([sum(bt[j] * Un[3 * i:3 * i + 3, j] for j in range(4)) for i in range(4)])
            pcs = alphas @ ccs
            if (pcs[0, 2] > 0) != (brg[0, 2] > 0):
                pcs = -pcs
            pc0, pw0 = pcs.sum(0) / n, pw.sum(0) / n
            CM = (pcs - pc0).T @ (pw - pw0)
            if not np.isfinite(CM.astype(np.float64)).all():  # a failed solve: the error is NaN and the candidate is never taken
                continue
            if dtype == np.float64 and not jacobi:
                cu, _, cvt = np.linalg.svd(CM)
            else:
                cu, _, cv = jacobi_svd(CM, dtype)
                cu = cu.copy()
                cu[:, 2] = np.cross(cu[:, 0], cu[:, 1])
                cvt = cv.T
            R = cu @ cvt
            if np.linalg.det(R.astype(np.float64)) < 0:
                R = cu @ np.diag(np.array([1, 1, -1], dtype)) @ cvt
            t = pc0 - R @ pw0
            err = reprojection_error(R, t, brg, pw)
            if err < best:
                best, R_best, t_best = float(err), R.astype(np.float64), t.astype(np.float64)
    return R_best, t_best, best, np.asarray(sv, np.float64)


def null_gap(sv):
    """smallest relative gap between neighbours among the four smallest singular values of M^T M (relative to the largest of the twelve)."""
    s = np.sort(np.asarray(sv, np.float64))[:4]
    return float(np.min(np.diff(s)) / np.max(sv))


# ------------------------------------------------------------------------------------------------ RANSAC
def check_inliers(R, t, bearings, pos_w, max_cos):
    """pnp_solver::check_inliers (:126-153): flags, num_inliers, cost, margin."""
    with np.errstate(all="ignore"):
        cos_angle = _cos_angles(np.asarray(R, np.float64), np.asarray(t, np.float64), bearings, pos_w)
        mce = np.asarray(max_cos, F32)
        flags = mce.astype(np.float64) < cos_angle
        cost = float(np.where(flags, 1 - cos_angle, (F32(1) - mce).astype(np.float64)).sum())
        margin = np.abs(cos_angle - mce.astype(np.float64)) / np.abs(mce.astype(np.float64))
    return flags, int(flags.sum()), cost, np.where(np.isfinite(margin), margin, np.inf)


def select(num_inliers, cost, min_num_inliers):
    """step 2-4 and the validity rule (:94-103) over the hypotheses of one problem, in iteration order: best iteration or -1."""
    min_cost, best = DBL_MAX, -1
    for it, (k, c) in enumerate(zip(num_inliers, cost)):
        if int(k) > min_num_inliers and min_cost > c:
            min_cost, best = c, it
    return best if min_cost < DBL_MAX else -1


def find_via_ransac(bearings, pos_w, octaves, scale_factors, samples, min_num_inliers=10, recompute=True, gn_iter=10, null_rot=None):
    """pnp_solver::find_via_ransac (:44-124) with the drawn samples given."""
    n = len(pos_w)
    out = dict(valid=False, R=np.zeros((3, 3)), t=np.zeros(3), is_inlier=np.zeros(n, bool), best_iter=-1)
    if n < 4 or n < min_num_inliers:
        return out
    mce = max_cos_errors(octaves, scale_factors)
    hyp = []
    for s in np.asarray(samples, np.int64):
        R, t, _, _ = compute_pose(bearings[s], pos_w[s], gn_iter, null_rot=null_rot)
        flags, num, cost, _ = check_inliers(R, t, bearings, pos_w, mce)
        hyp.append((R, t, flags, num, cost))
    best = select([h[3] for h in hyp], [h[4] for h in hyp], min_num_inliers)
    if best < 0:
        return out
    R, t, flags = hyp[best][:3]
    if recompute:
        R, t, _, _ = compute_pose(bearings[flags], pos_w[flags], gn_iter)
    return dict(valid=True, R=R, t=t, is_inlier=flags, best_iter=best)


def draw_samples(rng, n, num_iter):
    """num_iter x 4 distinct indices below n (any generator serves: the table is an input of the device)."""
    return np.stack([rng.choice(n, 4, replace=False) for _ in range(num_iter)]).astype(np.uint32) if n >= 4 else np.zeros((num_iter, 4), np.uint32)


# ------------------------------------------------------------------------------------------------ planted problems
def planted(seed, n, kind="pinhole", noise=0.0, outliers=0.0, octaves="mixed"):
    """n 2D-3D matches of a planted pose.  kind: pinhole (bearings in a 90 degree cone, z > 0), equirect (the camera looks backwards: bearings
    with z < 0, the sign flip of compute_pcs), coplanar (landmarks on one plane: the 1e-6 pseudo-inverse rule), far (|pos_w| ~ 1e3).
    noise: rotation of every bearing by about that many radians; outliers: share of matches whose bearing is replaced by a random one."""
    rng = np.random.default_rng(seed)
    R = rodrigues(rng.normal(size=3) * 0.4)
    pc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)
    if kind == "coplanar":
        pc[:, 2] = 5.0 + 0.3 * pc[:, 0] - 0.2 * pc[:, 1]
    if kind == "equirect":
        pc[:, 2] = -pc[:, 2]
    centre = np.array([1e3, -4e2, 7e2]) if kind == "far" else rng.normal(size=3)
    pw = (pc @ R) + centre           # pos_c = R (pos_w - centre)
    t = -R @ centre
    pc = pw @ R.T + t
    brg = pc / np.linalg.norm(pc, axis=1, keepdims=True)
    if noise > 0:
        brg = brg + rng.normal(size=(n, 3)) * noise
        brg /= np.linalg.norm(brg, axis=1, keepdims=True)
    is_out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        is_out[rng.choice(n, k, replace=False)] = True
        rnd = np.stack([rng.uniform(-0.5, 0.5, k), rng.uniform(-0.4, 0.4, k), np.ones(k)], 1)
        rnd[:, 2] *= -1.0 if kind == "equirect" else 1.0
        brg[is_out] = rnd / np.linalg.norm(rnd, axis=1, keepdims=True)
    oct_ = rng.integers(0, 8, n).astype(np.int32) if octaves == "mixed" else np.zeros(n, np.int32)
    return dict(name=f"{kind}_n{n}_s{seed}", bearings=np.ascontiguousarray(brg), pos_w=np.ascontiguousarray(pw), octaves=oct_, R=R, t=t, planted_outlier=is_out,
                scale_factors=orb_scale_factors())


KINDS = ("pinhole", "equirect", "coplanar", "far")


UNIQUE_KINDS = ("pinhole", "equirect", "far")  # coplanar landmarks leave alpha_3 = 0: three columns of M vanish and the null space has no unique basis


def pose_sets(noise, per_size=3):
    """over-determined sets for svgpu_pnp_compute_pose: every kind with a unique pose x OVERDETERMINED sizes x per_size seeds."""
    out = []
    for ki, kind in enumerate(UNIQUE_KINDS):
        for n in OVERDETERMINED:
            for s in range(per_size):
                out.append(planted(1000 * ki + 10 * n + s, n, kind, noise=noise))
    return out


def concatenate(problems):
    """flat arrays and offsets of a batch."""
    off = np.concatenate([[0], np.cumsum([len(p["pos_w"]) for p in problems])]).astype(np.int32)
    cat = lambda k, w, t: np.concatenate([np.asarray(p[k], t).reshape(-1, *w) for p in problems]) if problems else np.zeros((0, *w), t)
    return off, cat("bearings", (3,), np.float64), cat("pos_w", (3,), np.float64), cat("octaves", (), np.int32)


def ransac_batch(k, seed=0, num_iter=30):
    """k problems of uneven sizes (MATCH_COUNTS and others), 20 % outliers, with an empty one and one below four matches when k >= 3."""
    sizes = [80, 0, 3, 300, 64, 65, 63, 5, 4, 120, 37, 200, 9, 150, 81, 11, 100]
    probs = []
    for j in range(k):
        n = 80 if k == 1 else sizes[j % len(sizes)]
        p = planted(seed + j, n, KINDS[j % len(KINDS)], outliers=0.2 if n >= 20 else 0.0) if n else dict(
            name="empty", bearings=np.zeros((0, 3)), pos_w=np.zeros((0, 3)), octaves=np.zeros(0, np.int32), R=np.eye(3), t=np.zeros(3),
            planted_outlier=np.zeros(0, bool), scale_factors=orb_scale_factors())
        p["samples"] = draw_samples(np.random.default_rng(seed + 100 + j), n, num_iter)
        probs.append(p)
    return probs


def fixed_null_rotations():
    """two fixed rotations of the four-dimensional null space (QR of seeded normal matrices)."""
    return [np.linalg.qr(np.random.default_rng(s).normal(size=(4, 4)))[0] for s in (11, 12)]


_OUTCOME = None


def outcome_problems(count=10):
    """Planted RANSAC problems (80 matches, 20 % outliers, noise-free inliers, 30 iterations, min_num_inliers 10) and the indices of those
    the restatement solves whatever the null-space basis: the selected hypothesis has the inlier flags of the planted pose under LAPACK's
    basis and two fixed rotations of it.  Computed once per process."""
    global _OUTCOME
    if _OUTCOME is None:
        probs, kept = [], []
        for j in range(count):
            p = planted(500 + j, 80, KINDS[j % len(KINDS)], outliers=0.2)
            p["samples"] = draw_samples(np.random.default_rng(900 + j), 80, 30)
            mce = max_cos_errors(p["octaves"], p["scale_factors"])
            p["planted_flags"], _, _, p["planted_margin"] = check_inliers(p["R"], p["t"], p["bearings"], p["pos_w"], mce)
            good = True
            for q in [None] + fixed_null_rotations():
                r = find_via_ransac(p["bearings"], p["pos_w"], p["octaves"], p["scale_factors"], p["samples"], 10, False, 10, q)
                good = good and r["valid"] and np.array_equal(r["is_inlier"], p["planted_flags"])
            probs.append(p)
            if good:
                kept.append(j)
        _OUTCOME = (kept, probs)
    return _OUTCOME
