"""Problems and the CPU yardstick for the two-view triangulator (svgpu_triangulate_two_views).

The yardstick is a restatement of module::two_view_triangulator::triangulate (module/two_view_triangulator.{h,cc}), of
solve::triangulator::triangulate (solve/triangulator.h:76-88) and of data::triangulate_stereo (data/common.cc:192-261) in numpy: fp64
elementwise arithmetic in the reference's operation order, np.float32 where the reference has `float`, the null vector from np.linalg.svd.
`restate` also returns, per match, the smallest relative distance of any compared quantity from its threshold (the "margin"), and can take
the null vector from an extended-precision (np.longdouble) one-sided Jacobi instead: that result calibrates the position tolerance.
numpy only; shared by tests/test_triangulation_problem_classes.py (CPU) and tests/test_gpu_triangulate.py (GPU)."""
import numpy as np

PERSPECTIVE, FISHEYE, EQUIRECTANGULAR, RADIAL_DIVISION = 0, 1, 2, 3
ACCEPTED, NO_MODE, DEPTH, REPROJECTION, SCALE, SKIPPED = 0, 1, 2, 3, 4, 255
LINEAR, STEREO_1, STEREO_2, NONE = 0, 1, 2, -1
F32 = np.float32
CHI_SQ_2D, CHI_SQ_3D = F32(5.99146), F32(7.81473)


def orb_tables(scale_factor=1.2, num_levels=8):
    """feature/orb_params.cc:41-71: fp32 recurrences."""
    sf = np.ones(num_levels, F32)
    for l in range(1, num_levels):
        sf[l] = F32(scale_factor) * sf[l - 1]
    return dict(scale_factor=float(F32(scale_factor)), scale_factors=sf, level_sigma_sq=(sf * sf).astype(F32))


def camera(model, cols=1280, rows=960, fx=700.0, fy=690.0, cx=640.5, cy=470.25, true_baseline=0.0, dist=()):
    if model == EQUIRECTANGULAR:
        fx = fy = cx = cy = 0.0
        true_baseline = 0.0
    return dict(model=model, cols=cols, rows=rows, fx=fx, fy=fy, cx=cx, cy=cy, dist=tuple(dist), focal_x_baseline=fx * true_baseline,
                true_baseline=true_baseline, bounds=(0.0, float(cols), 0.0, float(rows)))


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def trans_wc(pose):
    """keyframe::set_pose_cw: -rot_wc * trans_cw, each element a left-to-right dot product."""
    P = np.asarray(pose, np.float64)
    return np.array([((-P[0, i]) * P[0, 3] + (-P[1, i]) * P[1, 3]) + (-P[2, i]) * P[2, 3] for i in range(3)])


def bearings_of(cam, xy):
    """camera::*::convert_keypoints_to_bearings (perspective.cc:117-122, equirectangular.cc:41-48)."""
    xy = np.asarray(xy, F32)
    if cam["model"] == EQUIRECTANGULAR:
        lon = ((xy[:, 0] / F32(cam["cols"])).astype(np.float64) - 0.5) * (2.0 * np.pi)
        lat = -((xy[:, 1] / F32(cam["rows"])).astype(np.float64) - 0.5) * np.pi
        return np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1)
    x = (xy[:, 0].astype(np.float64) - cam["cx"]) / cam["fx"]
    y = (xy[:, 1].astype(np.float64) - cam["cy"]) / cam["fy"]
    l2 = np.sqrt(x * x + y * y + 1.0)
    return np.stack([x / l2, y / l2, 1.0 / l2], 1)


def project(cam, pose, pw):
    """camera::*::reproject_to_image on fp64 arrays: (rx, ry, x_right as float32, pos_c); behind-the-camera points of the pinhole
    family keep rx = ry = 0 (the reference leaves them unset; the depth gate has rejected such a match before)."""
    P = np.asarray(pose, np.float64)
    X = _dot3(P[0, 0], P[0, 1], P[0, 2], pw[:, 0], pw[:, 1], pw[:, 2]) + P[0, 3]
    Y = _dot3(P[1, 0], P[1, 1], P[1, 2], pw[:, 0], pw[:, 1], pw[:, 2]) + P[1, 3]
    Z = _dot3(P[2, 0], P[2, 1], P[2, 2], pw[:, 0], pw[:, 1], pw[:, 2]) + P[2, 3]
    with np.errstate(all="ignore"):
        if cam["model"] == EQUIRECTANGULAR:
            nrm = np.sqrt((X * X + Y * Y) + Z * Z)
            bx, by, bz = X / nrm, Y / nrm, Z / nrm
            lat, lon = -np.arcsin(by), np.arctan2(bx, bz)
            rx = cam["cols"] * (0.5 + lon / (2.0 * np.pi))
            ry = cam["rows"] * (0.5 - lat / np.pi)
            xr = np.zeros(len(pw), F32)
        else:
            ok = Z > 0.0
            z_inv = 1.0 / np.where(ok, Z, 1.0)
            rx = np.where(ok, cam["fx"] * X * z_inv + cam["cx"], 0.0)
            ry = np.where(ok, cam["fy"] * Y * z_inv + cam["cy"], 0.0)
            xr = np.where(ok, rx - cam["focal_x_baseline"] * z_inv, 0.0).astype(F32)
    return rx, ry, xr, np.stack([X, Y, Z], 1)


# ------------------------------------------------------------------------------------------------ null vector of A
def build_A(b1, b2, P1, P2):
    """solve/triangulator.h:77-81, fp64: A.row(0) = bearing_1(0) * cam_pose_1.row(2) - bearing_1(2) * cam_pose_1.row(0) ..."""
    A = np.empty((len(b1), 4, 4))
    A[:, 0, :] = b1[:, 0:1] * P1[2][None, :] - b1[:, 2:3] * P1[0][None, :]
    A[:, 1, :] = b1[:, 1:2] * P1[2][None, :] - b1[:, 2:3] * P1[1][None, :]
    A[:, 2, :] = b2[:, 0:1] * P2[2][None, :] - b2[:, 2:3] * P2[0][None, :]
    A[:, 3, :] = b2[:, 1:2] * P2[2][None, :] - b2[:, 2:3] * P2[1][None, :]
    return A


def null_svd(A):
    """svd.matrixV().col(3), dehomogenised (fp64 LAPACK)."""
    if len(A) == 0:
        return np.zeros((0, 3))
    v = np.linalg.svd(A)[2][:, 3, :]
    with np.errstate(all="ignore"):
        return v[:, :3] / v[:, 3:4]


def null_jacobi(A, dtype=np.longdouble, sweeps=30):
    """One-sided (Hestenes) Jacobi on the columns of the fp64 matrix A, carried out in `dtype`; the column of V whose rotated column of A
    is the shortest, dehomogenised and rounded to fp64."""
    if len(A) == 0:
        return np.zeros((0, 3))
    a = np.asarray(A).astype(dtype).copy()  # a[m, r, c]
    v = np.broadcast_to(np.eye(4, dtype=dtype), a.shape).copy()
    eps = np.finfo(dtype).eps
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            any_rot = False
            for p in range(3):
                for q in range(p + 1, 4):
                    alpha = (a[:, :, p] ** 2).sum(1)
                    beta = (a[:, :, q] ** 2).sum(1)
                    gamma = (a[:, :, p] * a[:, :, q]).sum(1)
                    rot = (gamma != 0) & (np.abs(gamma) > eps * np.sqrt(alpha * beta))
                    if not rot.any():
                        continue
                    any_rot = True
                    g = np.where(rot, gamma, dtype(1))
                    zeta = (beta - alpha) / (2 * g)
                    t = np.where(zeta >= 0, dtype(1), dtype(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = 1 / np.sqrt(1 + t * t)
                    s = c * t
                    c, s = np.where(rot, c, dtype(1))[:, None], np.where(rot, s, dtype(0))[:, None]
                    for M in (a, v):
                        mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                        M[:, :, p] = c * mp - s * mq
                        M[:, :, q] = s * mp + c * mq
            if not any_rot:
                break
        j = (a ** 2).sum(1).argmin(1)
        x = v[np.arange(len(a)), :, j]
        return (x[:, :3] / x[:, 3:4]).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the restatement
def _rel(a, b):
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.where(np.isfinite(d), d, np.inf)


def _side(view, idx):
    n = len(idx)
    xy = np.asarray(view["xy"], F32).reshape(-1, 2)[idx]
    xr = np.full(n, -1, F32) if view.get("xright") is None else np.asarray(view["xright"], F32)[idx]
    dp = np.full(n, -1, F32) if view.get("depth") is None else np.asarray(view["depth"], F32)[idx]
    return xy, xr, dp, np.asarray(view["bearings"], np.float64).reshape(-1, 3)[idx], np.asarray(view["octave"])[idx]


def _stereo_point(view, xy, depth):
    """data::triangulate_stereo: (x - cx_) * depth * fx_inv_ is a double expression rounded to `const float`."""
    cam, P = view["cam"], np.asarray(view["pose_cw"], np.float64)
    ok = depth > 0
    if cam["model"] == EQUIRECTANGULAR:  # never reached with a stereo keypoint: the entry point refuses the combination
        return np.zeros((len(depth), 3))
    fx_inv, fy_inv = 1.0 / cam["fx"], 1.0 / cam["fy"]
    ux = ((xy[:, 0].astype(np.float64) - cam["cx"]) * depth.astype(np.float64) * fx_inv).astype(F32).astype(np.float64)
    uy = ((xy[:, 1].astype(np.float64) - cam["cy"]) * depth.astype(np.float64) * fy_inv).astype(F32).astype(np.float64)
    uz = depth.astype(np.float64)
    c = trans_wc(P)
    out = np.stack([_dot3(P[0, i], P[1, i], P[2, i], ux, uy, uz) + c[i] for i in range(3)], 1)
    return np.where(ok[:, None], out, 0.0)


def restate(view1, view2, tables, idx1, idx2, rays_parallax_deg_thr=1.0, null="svd"):
    """Returns dict(pos_w, status, branch, margin).  `null`: "svd" (np.linalg.svd, the yardstick) or "longdouble"."""
    idx1, idx2 = np.asarray(idx1, np.int64), np.asarray(idx2, np.int64)
    M = len(idx1)
    P1, P2 = np.asarray(view1["pose_cw"], np.float64)[:3, :4], np.asarray(view2["pose_cw"], np.float64)[:3, :4]
    xy1, xr1, dp1, b1, o1 = _side(view1, idx1)
    xy2, xr2, dp2, b2, o2 = _side(view2, idx2)
    st1, st2 = xr1 >= 0, xr2 >= 0
    w1 = [_dot3(P1[0, i], P1[1, i], P1[2, i], b1[:, 0], b1[:, 1], b1[:, 2]) for i in range(3)]
    w2 = [_dot3(P2[0, i], P2[1, i], P2[2, i], b2[:, 0], b2[:, 1], b2[:, 2]) for i in range(3)]
    cos_rays = _dot3(w1[0], w1[1], w1[2], w2[0], w2[1], w2[2])
    cs1 = np.where(st1, np.cos(2.0 * np.arctan2(view1["true_baseline"] / 2.0, dp1.astype(np.float64))), 2.0)
    cs2 = np.where(st2, np.cos(2.0 * np.arctan2(view2["true_baseline"] / 2.0, dp2.astype(np.float64))), 2.0)
    cs = np.minimum(cs1, cs2)
    thr = np.float64(F32(np.cos(np.float64(F32(rays_parallax_deg_thr)) * np.pi / 180.0)))
    mono = ~st1 & ~st2
    bound = np.where(mono, thr, cs)
    linear = (0.0 < cos_rays) & (cos_rays < bound)
    s1 = ~linear & st1 & (cs1 < cs2)
    s2 = ~linear & ~s1 & st2 & (cs2 < cs1)
    branch = np.where(linear, LINEAR, np.where(s1, STEREO_1, np.where(s2, STEREO_2, NONE)))
    margin = np.minimum(np.abs(cos_rays), _rel(cos_rays, bound))
    margin = np.where(~linear & (st1 | st2), np.minimum(margin, _rel(cs1, cs2)), margin)

    pos = np.zeros((M, 3))
    A = build_A(b1[linear], b2[linear], P1, P2)
    pos[linear] = null_svd(A) if null == "svd" else null_jacobi(A)
    pos[s1] = _stereo_point(view1, xy1[s1], dp1[s1])
    pos[s2] = _stereo_point(view2, xy2[s2], dp2[s2])

    status = np.where(branch == NONE, NO_MODE, ACCEPTED).astype(np.uint8)
    tb = tables
    live = status == ACCEPTED
    # check_depth_is_positive of both, then check_reprojection_error of both
    proj = [project(view1["cam"], P1, pos), project(view2["cam"], P2, pos)]
    dmargin = np.full(M, np.inf)
    dfail = np.zeros(M, bool)
    for (view, (rx, ry, xr, pc)) in zip((view1, view2), proj):
        if view["cam"]["model"] != EQUIRECTANGULAR:
            with np.errstate(all="ignore"):
                nrm = np.sqrt((pc ** 2).sum(1))
                dmargin = np.minimum(dmargin, np.where(nrm > 0, np.abs(pc[:, 2]) / np.where(nrm > 0, nrm, 1.0), np.inf))
            dfail |= ~(0 < pc[:, 2])
    margin = np.where(live, np.minimum(margin, dmargin), margin)
    status[live & dfail] = DEPTH
    live = status == ACCEPTED
    rfail = np.zeros(M, bool)
    rmargin = np.full(M, np.inf)
    for (view, (rx, ry, xr, pc), xy, xrk, stk, ok) in zip((view1, view2), proj, (xy1, xy2), (xr1, xr2), (st1, st2), (o1, o2)):
        sig = np.asarray(tb["level_sigma_sq"], F32)[ok]
        with np.errstate(all="ignore"):
            ex, ey = rx - xy[:, 0].astype(np.float64), ry - xy[:, 1].astype(np.float64)
            sq = ex * ex + ey * ey
            exr = (xr - xrk).astype(F32)
            lhs = np.where(stk, (CHI_SQ_3D * sig).astype(np.float64), (CHI_SQ_2D * sig).astype(np.float64))
            rhs = np.where(stk, sq + (exr * exr).astype(F32).astype(np.float64), sq)
            rfail |= lhs < rhs
        rmargin = np.minimum(rmargin, _rel(lhs, rhs))
    margin = np.where(live, np.minimum(margin, rmargin), margin)
    status[live & rfail] = REPROJECTION
    live = status == ACCEPTED
    # check_scale_factors
    c1, c2 = trans_wc(P1), trans_wc(P2)
    d1 = np.sqrt(((pos[:, 0] - c1[0]) ** 2 + (pos[:, 1] - c1[1]) ** 2) + (pos[:, 2] - c1[2]) ** 2)
    d2 = np.sqrt(((pos[:, 0] - c2[0]) ** 2 + (pos[:, 1] - c2[1]) ** 2) + (pos[:, 2] - c2[2]) ** 2)
    zero = (d1 == 0) | (d2 == 0)
    sf = np.asarray(tb["scale_factors"], F32)
    ratio_factor = np.float64(F32(2.0) * max(F32(view1["scale_factor"]), F32(view2["scale_factor"])))
    with np.errstate(all="ignore"):
        ratio_dists = d2 / d1
        ratio_octave = (sf[o1] / sf[o2]).astype(F32).astype(np.float64)
        qa, qb = ratio_octave / ratio_dists, ratio_dists / ratio_octave
        sfail = zero | ~((qa < ratio_factor) & (qb < ratio_factor))
        smargin = np.where(zero, np.inf, np.minimum(_rel(qa, ratio_factor), _rel(qb, ratio_factor)))
    margin = np.where(live, np.minimum(margin, smargin), margin)
    status[live & sfail] = SCALE
    return dict(pos_w=pos, status=status, branch=branch, margin=margin)


def restate_problem(p, null="svd"):
    """restate() on a problem of this module, in either input form; unmatched entries of the matched_2_in_1 form get SKIPPED."""
    if p.get("idx2") is not None:
        return restate(p["view1"], p["view2"], p["tables"], p["idx1"], p["idx2"], p["deg_thr"], null)
    m21 = np.asarray(p["idx1"])
    has = m21 >= 0
    r = restate(p["view1"], p["view2"], p["tables"], np.flatnonzero(has), m21[has], p["deg_thr"], null)
    out = dict(pos_w=np.zeros((len(m21), 3)), status=np.full(len(m21), SKIPPED, np.uint8), branch=np.full(len(m21), NONE), margin=np.full(len(m21), np.inf))
    for k in out:
        out[k][has] = r[k]
    return out


# ------------------------------------------------------------------------------------------------ generators
def _view(cam, pose, xy, octave, tables, xright=None, depth=None):
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    return dict(cam=cam, pose_cw=np.ascontiguousarray(pose, np.float64), true_baseline=cam["true_baseline"], xy=xy, octave=np.ascontiguousarray(octave, np.int32),
                bearings=bearings_of(cam, xy), xright=xright, depth=depth, scale_factor=tables["scale_factor"])


def _pose(rng, rot_deg, t):
    w = rng.normal(0, 1, 3)
    w *= np.deg2rad(rot_deg) / np.linalg.norm(w)
    R = rodrigues(w)
    return np.concatenate([R, (-R @ np.asarray(t, np.float64))[:, None]], 1)  # camera centre at t


def _points(rng, cam, pose, n, dmin, dmax):
    """n world points seen by `cam` at `pose`, distances log-uniform in [dmin, dmax]."""
    d = np.exp(rng.uniform(np.log(dmin), np.log(dmax), n))
    if cam["model"] == EQUIRECTANGULAR:
        v = rng.normal(0, 1, (n, 3))
        pc = v / np.linalg.norm(v, axis=1)[:, None] * d[:, None]
    else:
        u, v = rng.uniform(40, cam["cols"] - 40, n), rng.uniform(40, cam["rows"] - 40, n)
        pc = np.stack([(u - cam["cx"]) / cam["fx"] * d, (v - cam["cy"]) / cam["fy"] * d, d], 1)
    R, t = pose[:, :3], pose[:, 3]
    return (pc - t) @ R  # R^T (pc - t)


def make_pair(seed, n, model1=PERSPECTIVE, model2=None, stereo=(False, False), centre2=(0.35, 0.02, -0.03), rot2_deg=2.0, dmin=1.5, dmax=60.0, noise=1.0,
              octave_delta=(-1, 0, 1), outliers=0.0, depth_noise=0.0, true_baseline=0.12, deg_thr=1.0, extra=40, form="pairs", drop_arrays=False, name=""):
    """A keyframe pair looking at n planted points: pixel noise of `noise` sigma times the octave's scale factor, octave pairs o2 = o1 + delta,
    a share of gross outliers; `extra` unmatched keypoints per side and shuffled keypoint order, so that idx1 / idx2 are not the identity."""
    rng = np.random.default_rng(seed)
    model2 = model1 if model2 is None else model2
    tb = orb_tables()
    cams = [camera(m, true_baseline=true_baseline if s else 0.0) for m, s in zip((model1, model2), stereo)]
    poses = [_pose(rng, 1.0, rng.normal(0, 0.05, 3)), None]
    poses[1] = _pose(rng, rot2_deg, trans_wc(poses[0]) + poses[0][:, :3].T @ np.asarray(centre2))
    pw = _points(rng, cams[0], poses[0], n, dmin, dmax)
    o1 = rng.integers(0, 8, n)
    o2 = np.clip(o1 + rng.choice(np.asarray(octave_delta), n), 0, 7)
    bad = rng.uniform(0, 1, n) < outliers
    views, idx = [], []
    for cam, pose, oc, st in zip(cams, poses, (o1, o2), stereo):
        rx, ry, _, pc = project(cam, pose, pw)
        sig = tb["scale_factors"][oc].astype(np.float64) * noise
        x = rx + rng.normal(0, 1, n) * sig + np.where(bad, rng.uniform(-120, 120, n), 0.0)
        y = ry + rng.normal(0, 1, n) * sig + np.where(bad, rng.uniform(-120, 120, n), 0.0)
        nt = n + extra
        perm = rng.permutation(nt)  # keypoint perm[j] holds planted point j
        xy = np.zeros((nt, 2), F32)
        xy[:, 0], xy[:, 1] = rng.uniform(0, cam["cols"], nt), rng.uniform(0, cam["rows"], nt)
        octave = rng.integers(0, 8, nt)
        xy[perm[:n], 0], xy[perm[:n], 1], octave[perm[:n]] = x, y, oc
        xright = depth = None
        if st:
            z = pc[:, 2] * (1.0 + depth_noise * rng.normal(0, 1, n))
            xright, depth = np.full(nt, -1, F32), np.full(nt, -1, F32)
            mono = rng.uniform(0, 1, n) < 0.1  # a stereo rig still has keypoints without a right match
            xright[perm[:n]] = np.where(mono, -1.0, np.maximum(x - cam["focal_x_baseline"] / z + rng.normal(0, 1, n) * sig, 0.0))
            depth[perm[:n]] = np.where(mono, -1.0, z)
        elif not drop_arrays:
            xright, depth = np.full(nt, -1, F32), np.full(nt, -1, F32)
        views.append(_view(cam, pose, xy, octave, tb, xright, depth))
        idx.append(perm[:n].astype(np.int32))
    p = dict(name=name, view1=views[0], view2=views[1], tables=tb, deg_thr=deg_thr, idx1=idx[0], idx2=idx[1], exact=False, planted=pw)
    if form == "matched_2_in_1":
        m21 = np.full(len(views[0]["octave"]), -1, np.int32)
        m21[idx[0]] = idx[1]
        p["idx1"], p["idx2"] = m21, None
    return p


def behind_one_camera(seed=31, n=400):
    """Camera 2 stands beyond the points and looks the same way: the two LINES meet at the planted point, which lies behind camera 2."""
    return make_pair(seed, n, centre2=(3.0, 0.2, 25.0), rot2_deg=1.0, dmin=6.0, dmax=14.0, octave_delta=(0,), name="behind_one_camera")


def exact_threshold_cases():
    """Classes built to sit ON a threshold, from exactly representable inputs: no exemption applies to them.
    a) equal stereo cosines: identical poses, identical keypoints, depth_1 == depth_2 -> neither stereo branch -> NO_MODE
    b) depth <= 0 with a stereo x_right: zero vector; identity pose -> pos_z == 0 -> DEPTH; camera 2 at t_z = 1 -> REPROJECTION
    c) zero distance: equirectangular keyframe 1 at the origin (no depth test), stereo keyframe 2 with depth 0 whose keypoint sits on the
       reprojection of the origin -> every earlier gate passes, cam_1_to_lm_dist == 0 -> SCALE"""
    tb = orb_tables()
    out = []
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    cam = camera(PERSPECTIVE, fx=512.0, fy=512.0, cx=640.0, cy=480.0, true_baseline=0.125)
    n = 64
    g = np.arange(n)
    xy = np.stack([320.0 + 8.0 * g, 200.0 + 4.0 * g], 1).astype(F32)
    octv = (g % 8).astype(np.int32)
    depth = (2.0 + 0.25 * (g % 16)).astype(F32)
    xr = (xy[:, 0] - F32(64.0) / depth).astype(F32)
    a = dict(name="equal_stereo_cosines", view1=_view(cam, I, xy, octv, tb, xr, depth), view2=_view(cam, I, xy, octv, tb, xr, depth), tables=tb, deg_thr=1.0,
             idx1=g.astype(np.int32), idx2=g.astype(np.int32), exact=True, expect=NO_MODE)
    out.append(a)
    mono = camera(PERSPECTIVE, fx=512.0, fy=512.0, cx=640.0, cy=480.0)
    d0 = np.where(g % 2 == 0, 0.0, -1.0).astype(F32)
    b1 = dict(name="nonpositive_depth_identity", view1=_view(cam, I, xy, octv, tb, np.abs(xr), d0), view2=_view(mono, I, xy, octv, tb), tables=tb, deg_thr=1.0,
              idx1=g.astype(np.int32), idx2=g.astype(np.int32), exact=True, expect=DEPTH)
    out.append(b1)
    T = I.copy()
    T[:, 3] = (0.5, 0.25, 1.0)
    b2 = dict(name="nonpositive_depth_shifted", view1=_view(cam, T, xy, octv, tb, np.abs(xr), d0), view2=_view(mono, T, xy, octv, tb), tables=tb, deg_thr=1.0,
              idx1=g.astype(np.int32), idx2=g.astype(np.int32), exact=True, expect=REPROJECTION)
    out.append(b2)
    eq = camera(EQUIRECTANGULAR, cols=2048, rows=1024)
    T2 = I.copy()
    T2[:, 3] = (0.0, 0.0, 1.0)
    xy2 = np.tile(np.array([[640.0, 480.0]], F32), (n, 1))  # the origin seen from camera 2: (cx, cy), x_right = cx - fxb * 1
    xr2 = np.full(n, 640.0 - 64.0, F32)
    xy1 = np.stack([100.0 + 16.0 * g, 300.0 + 2.0 * g], 1).astype(F32)
    c = dict(name="zero_distance", view1=_view(eq, I, xy1, octv, tb), view2=_view(cam, T2, xy2, octv, tb, xr2, d0), tables=tb, deg_thr=1.0, idx1=g.astype(np.int32),
             idx2=g.astype(np.int32), exact=True, expect=SCALE)
    c["view2"]["depth"] = np.zeros(n, F32)
    out.append(c)
    return out


def problem_classes():
    """name -> list of problems.  Seeds fixed."""
    C = {}
    C["perspective_mono"] = [make_pair(1, 3000, name="perspective_mono")]
    C["fisheye"] = [make_pair(2, 2000, FISHEYE, name="fisheye")]
    C["radial_division"] = [make_pair(3, 2000, RADIAL_DIVISION, name="radial_division")]
    C["equirectangular"] = [make_pair(4, 2000, EQUIRECTANGULAR, name="equirectangular", dmin=2.0, dmax=40.0)]
    forward = dict(centre2=(0.08, 0.0, 0.25), depth_noise=0.02, dmin=1.5, dmax=12.0)
    C["stereo_stereo"] = [make_pair(5, 3000, stereo=(True, True), name="stereo_stereo", **forward)]
    C["stereo_mono"] = [make_pair(6, 2000, stereo=(True, False), name="stereo_mono", **forward)]
    C["mono_stereo"] = [make_pair(7, 2000, stereo=(False, True), name="mono_stereo", drop_arrays=True, **forward)]
    C["parallax_straddle"] = [make_pair(8, 3000, dmin=10.0, dmax=40.0, name="parallax_straddle"),
                              make_pair(9, 1000, dmin=10.0, dmax=40.0, deg_thr=0.5, name="parallax_straddle_half_degree")]
    C["behind_one_camera"] = [behind_one_camera()]
    C["gross_outliers"] = [make_pair(10, 3000, outliers=0.3, name="gross_outliers"),
                           make_pair(11, 2000, stereo=(True, True), outliers=0.3, name="gross_outliers_stereo", **forward)]
    C["octave_straddle"] = [make_pair(12, 3000, octave_delta=(-5, -4, 4, 5), noise=0.3, name="octave_straddle")]
    # identical poses: a degenerate geometry (A has rank 2); the noise is kept well below the parallax threshold so that the parallax gate
    # rejects every match and no arbitrary null vector is ever compared
    C["identical_poses"] = [make_pair(13, 1000, centre2=(0.0, 0.0, 0.0), rot2_deg=0.0, noise=0.3, name="identical_poses")]
    C["sizes"] = [make_pair(20 + i, m, name=f"size_{m}", extra=5) for i, m in enumerate((0, 1, 63, 64, 65))]
    C["size_20000"] = [make_pair(30, 20000, name="size_20000")]
    C["matched_2_in_1"] = [make_pair(15, 1500, form="matched_2_in_1", extra=400, name="matched_2_in_1"),
                           make_pair(16, 800, stereo=(True, True), form="matched_2_in_1", extra=300, name="matched_2_in_1_stereo", **forward)]
    C["absent_arrays"] = [make_pair(17, 1000, drop_arrays=True, name="absent_arrays")]
    C["exact_thresholds"] = exact_threshold_cases()
    return C


def closed_form(seed=40, n=2000):
    """Noise-free bearings of planted points (bearings computed in fp64 from the exact projections, not from float32 pixels)."""
    rng = np.random.default_rng(seed)
    tb = orb_tables()
    cam = camera(PERSPECTIVE)
    P1 = _pose(rng, 3.0, (0.0, 0.0, 0.0))
    P2 = _pose(rng, 5.0, (0.6, -0.1, 0.05))
    pw = _points(rng, cam, P1, n, 2.0, 30.0)
    bs = []
    for P in (P1, P2):
        pc = project(cam, P, pw)[3]
        bs.append(pc / np.linalg.norm(pc, axis=1)[:, None])
    return dict(P1=P1, P2=P2, b1=bs[0], b2=bs[1], planted=pw, tables=tb)
