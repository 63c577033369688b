"""Problems and the CPU restatement for svgpu_new_landmarks_batch (the loop of mapping_module::create_new_landmarks, mapping_module.cc:275-341):
numpy and the CPU oracle only.

A problem is a dict: side1 / side2[k] (matcher sides: desc, angle, has_lm, node), view1 / neighbours[k] (the triangulator's views of
tests/triangulation_problems.py: cam, pose_cw, true_baseline, xy, octave, bearings, xright, depth, scale_factor), E_12 (K x 3 x 3),
epipole_in_2 (K x 3), valid_epipole (K), active (K or None), tables, lowe_ratio, residual_rad_thr, deg_thr.

`chain` is the reference loop restated: per neighbour the matcher oracle that tests/bucket_batch_problems.py uses (O.match_for_triangulation)
with has_lm1 = the keypoints taken so far, then triangulation_problems.restate on its matches, then `taken |= accepted`.  carry=False is the
composition of the two existing batch calls: every neighbour sees taken_0.

The scenes: one current keyframe and K neighbours looking at planted world points.  A point's keypoints carry the point's random
descriptor with a few bits flipped (twins are at most 12 bits apart, strangers about 128), so the matches are the planted ones; `shadows`
are extra keypoints of the current keyframe, behind every planted one in index order, that sit on a planted keypoint's pixel with its
descriptor 12 more bits away and have no twin of their own: while the planted keypoint is a query it claims the neighbour's twin first."""
import functools

import numpy as np

from oracle import oracle as O
from tests import triangulation_problems as T

F32 = np.float32
CLASSES = ["order_effect", "rejected_stay", "inactive_middle", "all_inactive", "all_taken_after_first", "empty_neighbour", "empty_current", "single",
           "robust", "stereo", "models", "buckets_64_65", "spill"]


def cand_lds_bytes(nq, nt, k=0):
    """A COPY of csrc/match_kernels.hip cand_lds_bytes (without counts) and, below, of CAND_LDS_BUDGET: this module runs without the library, so
    it cannot ask sv_cand_replay_form.  tests/test_gpu_new_landmarks.py asserts through svgpu_selftest_cand_replay_form that the sizes derived
    from the copy still reach the forms they are meant for; a drift of the copy fails there, not in the CPU class test."""
    return (nt + nq + nq + 1) * 4 + nq * k * 4 + 2 * ((nt + 3) & ~3) + ((nq + 3) & ~3) + 16


CAND_LDS_BUDGET = 150 * 1024
SPILL_N1 = 300
SPILL_N2 = next(n for n in range(1000, 1 << 20, 500) if cand_lds_bytes(SPILL_N1, n) > CAND_LDS_BUDGET)  # the replay's tables leave LDS


def _flip(rng, desc, k):
    """every row of desc (n x 32 bytes) with exactly k[row] bits flipped"""
    bits = np.unpackbits(desc, axis=1)
    order = rng.random(bits.shape).argsort(1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(256)[None, :].repeat(len(bits), 0), 1)
    bits ^= (rank < np.asarray(k)[:, None]).astype(np.uint8)
    return np.packbits(bits, axis=1)


def _cross(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def make(seed, n_pts, centres, models=None, stereo=False, extra1=30, extras2=None, with_nodes=True, shadows=0, bad0=0, taken_frac=0.0,
         residual_rad_thr=0.01, active=None, n_nodes=12, sizes2=None, name=""):
    """centres[k]: the camera centre of neighbour k in the current keyframe's frame.  sizes2[k] (optional): how many planted points neighbour k
    sees (its first ones).  bad0: in neighbour 0, four groups of bad0 planted keypoints each that the matcher still pairs (the class widens
    residual_rad_thr) and the triangulator rejects: far points (NO_MODE), diverging rays (DEPTH), displaced (REPROJECTION), octaves 5 apart (SCALE)."""
    rng = np.random.default_rng(seed)
    K = len(centres)
    tb = T.orb_tables()
    sf = tb["scale_factors"].astype(np.float64)
    models = models or [T.PERSPECTIVE] * (K + 1)
    base_line = 0.12 if stereo else 0.0
    cams = [T.camera(m, true_baseline=0.0 if m == T.EQUIRECTANGULAR else base_line) for m in models]
    pose1 = T._pose(rng, 1.0, rng.normal(0, 0.05, 3))
    c1, R1 = T.trans_wc(pose1), pose1[:, :3]
    poses = [pose1] + [T._pose(rng, 2.0, c1 + R1.T @ np.asarray(c, np.float64)) for c in centres]
    pw = T._points(rng, cams[0], pose1, n_pts, 2.0, 12.0 if stereo else 40.0)
    grp = {}
    if bad0:
        assert n_pts >= 8 * bad0
        for g, key in enumerate(("no_mode", "depth", "reproj", "scale")):
            grp[key] = np.arange(g * bad0, (g + 1) * bad0)
        far = grp["no_mode"]  # 3 000 times farther along the same ray of the current keyframe: no parallax against any neighbour
        pw[far] = c1 + (pw[far] - c1) * 3000.0
        near = np.arange(bad0, 4 * bad0)  # the other three groups at 4 m: enough parallax for the two-camera mode against every neighbour
        pw[near] = c1 + (pw[near] - c1) * (4.0 / np.linalg.norm(pw[near] - c1, axis=1))[:, None]
    base_desc = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    o1 = rng.integers(0, 6, n_pts)
    if bad0:
        o1[3 * bad0:4 * bad0] = rng.integers(0, 3, bad0)   # room for an octave 5 levels up
    pt_node = (np.arange(n_pts) % n_nodes).astype(np.int32)
    pt_angle = rng.uniform(0, 360, n_pts)
    sides, views, kp_of_pt = [], [], []
    for v in range(K + 1):
        cam, pose = cams[v], poses[v]
        seen = n_pts if (v == 0 or sizes2 is None) else sizes2[v - 1]
        extra = extra1 + shadows if v == 0 else (extras2[v - 1] if extras2 is not None else 25)
        rx, ry, _, pc = T.project(cam, pose, pw[:seen])
        oc = o1[:seen] if v == 0 else np.clip(o1[:seen] + rng.integers(-1, 2, seen), 0, 7)
        sig = sf[oc] * 0.4
        x, y = rx + rng.normal(0, 1, seen) * sig, ry + rng.normal(0, 1, seen) * sig
        if v == 1 and bad0:
            d, r, s = grp["depth"], grp["reproj"], grp["scale"]
            x[d] += np.sign(centres[0][0] if centres[0][0] else 1.0) * 90.0   # against the disparity and beyond it: the rays diverge
            ang = rng.uniform(0, 2 * np.pi, len(r))
            x[r], y[r] = x[r] + 45.0 * np.cos(ang), y[r] + 45.0 * np.sin(ang)
            oc = oc.copy()
            oc[s] = o1[s] + 5
            x[s], y[s] = rx[s] + rng.normal(0, 0.1, len(s)), ry[s] + rng.normal(0, 0.1, len(s))
        nt = seen + extra
        planted = nt - shadows if v == 0 else nt
        perm = rng.permutation(planted)  # keypoint perm[j] holds planted point j
        xy = np.zeros((nt, 2), F32)
        xy[:, 0], xy[:, 1] = rng.uniform(0, cam["cols"], nt), rng.uniform(0, cam["rows"], nt)
        octave = rng.integers(0, 8, nt)
        kp = perm[:seen]
        xy[kp, 0], xy[kp, 1], octave[kp] = x, y, oc
        desc = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        desc[kp] = _flip(rng, base_desc[:seen], rng.integers(0, 7, seen))
        node = rng.integers(0, n_nodes + 3, nt).astype(np.int32)
        node[rng.uniform(0, 1, nt) < 0.05] = -1   # clutter without a node
        node[kp] = pt_node[:seen]
        angle = rng.uniform(0, 360, nt).astype(F32)
        angle[kp] = ((pt_angle[:seen] + rng.normal(0, 3, seen)) % 360.0).astype(F32)   # twins agree in orientation; a few sit across the 0 / 360 seam
        xright = depth = None
        if stereo and cam["model"] != T.EQUIRECTANGULAR:
            z = pc[:, 2] * (1.0 + 0.02 * rng.normal(0, 1, seen))
            xright, depth = np.full(nt, -1, F32), np.full(nt, -1, F32)
            mono = rng.uniform(0, 1, seen) < 0.1
            xright[kp] = np.where(mono, -1.0, np.maximum(x - cam["focal_x_baseline"] / z + rng.normal(0, 1, seen) * sig, 0.0))
            depth[kp] = np.where(mono, -1.0, z)
        if v == 0 and shadows:  # on the pixel of planted points 8 * bad0 .. (never one of the rejected groups), 12 more bits away, same node and octave
            src = kp[8 * bad0:8 * bad0 + shadows]
            sh = np.arange(nt - shadows, nt)
            xy[sh], octave[sh], node[sh], angle[sh] = xy[src], octave[src], node[src], angle[src]
            desc[sh] = _flip(rng, desc[src], np.full(shadows, 12))
            if xright is not None:
                xright[sh], depth[sh] = xright[src], depth[src]
        has_lm = (rng.uniform(0, 1, nt) < (taken_frac if v == 0 else 0.1)).astype(np.uint8)
        if v > 0:
            has_lm[kp] = 0
        view = T._view(cam, pose, xy, octave, tb, xright, depth)
        views.append(view)
        sides.append(dict(desc=desc, angle=angle, has_lm=has_lm, node=node if with_nodes else None))
        kp_of_pt.append(kp)
    E, epi, ve = np.zeros((K, 3, 3)), np.zeros((K, 3)), np.zeros(K, np.int32)
    for k in range(K):
        P2, cam2 = poses[k + 1], cams[k + 1]
        R12 = R1 @ P2[:, :3].T
        E[k] = _cross(pose1[:, 3] - R12 @ P2[:, 3]) @ R12
        p = P2[:, :3] @ c1 + P2[:, 3]
        epi[k] = p / np.linalg.norm(p)
        if cam2["model"] == T.EQUIRECTANGULAR:
            ve[k] = 1
        elif p[2] > 0:
            u, w = cam2["fx"] * p[0] / p[2] + cam2["cx"], cam2["fy"] * p[1] / p[2] + cam2["cy"]
            ve[k] = int(0 < u < cam2["cols"] and 0 < w < cam2["rows"])
    return dict(name=name, side1=sides[0], view1=views[0], side2=sides[1:], neighbours=views[1:], E_12=E, epipole_in_2=epi, valid_epipole=ve,
                active=None if active is None else np.asarray(active, np.uint8), tables=tb, lowe_ratio=0.8, residual_rad_thr=residual_rad_thr, deg_thr=1.0,
                kp_of_pt=kp_of_pt, groups=grp, shadows=np.arange(len(sides[0]["desc"]) - shadows, len(sides[0]["desc"])), bad0=bad0)


SIDE, FWD, BACK, UP = (0.35, 0.02, -0.03), (0.08, 0.0, 0.25), (-0.3, 0.05, 0.1), (0.05, -0.4, 0.02)


@functools.lru_cache(maxsize=None)
def problem(name):
    return globals()["_" + name]()


def _order_effect():  # (a) and (f, bow_tree)
    return make(1, 200, [SIDE, BACK, UP], shadows=12, taken_frac=0.1, name="order_effect")


def _rejected_stay():  # (b): the wide epipolar gate lets the matcher pair what the triangulator then rejects
    return make(2, 220, [SIDE, BACK], bad0=6, shadows=6, residual_rad_thr=0.25, name="rejected_stay")


def _inactive_middle():  # (c)
    return make(3, 150, [SIDE, BACK, UP], active=[1, 0, 1], shadows=8, name="inactive_middle")


def _all_inactive():  # (c)
    return make(4, 64, [SIDE, BACK], active=[0, 0], name="all_inactive")


def _all_taken_after_first():  # (d): whatever neighbour 0 leaves without a landmark held one before the call
    p = make(5, 180, [SIDE, BACK, UP], extra1=0, name="all_taken_after_first")
    first = chain(dict(p, side2=p["side2"][:1], neighbours=p["neighbours"][:1], E_12=p["E_12"][:1], epipole_in_2=p["epipole_in_2"][:1],
                       valid_epipole=p["valid_epipole"][:1], side1=dict(p["side1"], has_lm=np.zeros(len(p["side1"]["desc"]), np.uint8))))
    p["side1"] = dict(p["side1"], has_lm=(first["status"][0] != T.ACCEPTED).astype(np.uint8))
    return p


def _empty_neighbour():  # (e): n2 == 0 between two neighbours
    p = make(6, 100, [SIDE, BACK, UP], shadows=5, name="empty_neighbour")
    none = np.zeros(0, np.int64)
    p["side2"][1] = {k: (None if v is None else v[none]) for k, v in p["side2"][1].items()}
    p["neighbours"][1] = dict(p["neighbours"][1], **{k: (None if p["neighbours"][1][k] is None else p["neighbours"][1][k][none]) for k in ("xy", "octave", "bearings", "xright", "depth")})
    return p


def _empty_current():  # (e): n1 == 0
    p = make(7, 64, [SIDE, BACK], name="empty_current")
    none = np.zeros(0, np.int64)
    p["side1"] = {k: (None if v is None else v[none]) for k, v in p["side1"].items()}
    p["view1"] = dict(p["view1"], **{k: (None if p["view1"][k] is None else p["view1"][k][none]) for k in ("xy", "octave", "bearings", "xright", "depth")})
    p["shadows"] = np.zeros(0, np.int64)
    return p


def _single():  # (e): K == 1
    return make(8, 120, [SIDE], taken_frac=0.2, name="single")


def _robust():  # (f): no node ids
    return make(9, 150, [SIDE, BACK, UP, FWD], with_nodes=False, shadows=10, taken_frac=0.1, name="robust")


def _stereo():  # (g): forward motion, little parallax: the triangulate_stereo branches
    return make(10, 200, [FWD, (0.02, 0.0, 0.1), SIDE], stereo=True, shadows=8, name="stereo")


def _models():  # (h)
    return make(11, 160, [SIDE, BACK, UP], models=[T.PERSPECTIVE, T.FISHEYE, T.EQUIRECTANGULAR, T.RADIAL_DIVISION], shadows=8, name="models")


def _buckets_64_65():  # (i): one node of neighbour 0 holds exactly 64 keypoints, of neighbour 1 exactly 65; taken_0 non-trivial
    p = make(12, 256, [SIDE, BACK], n_nodes=4, extra1=20, extras2=[44, 44], shadows=6, taken_frac=0.3, name="buckets_64_65")
    for k, want in enumerate((64, 65)):
        node = p["side2"][k]["node"]
        spare = np.setdiff1d(np.arange(len(node)), p["kp_of_pt"][k + 1])   # clutter keypoints: their node is free to set
        node[spare] = 50
        have = int((node == 0).sum())
        assert have <= want <= have + len(spare)
        node[spare[:want - have]] = 0
        assert (node == 0).sum() == want
    return p


def _spill():  # (j): the middle neighbour is large enough for the global-memory replay (SPILL_N2 from cand_lds_bytes)
    return make(13, SPILL_N1 - 30, [SIDE, BACK, UP], extra1=24, shadows=6, extras2=[25, SPILL_N2 - (SPILL_N1 - 30), 25], n_nodes=40, name="spill")


# ------------------------------------------------------------------------------------------------ the restatement
def chain(p, check_orientation=True, carry=True, null="svd"):
    """The loop :286-340 restated.  Returns dict(matched_2_in_1 K x n1, pos_w, status, margin, branch, num_matches, num_accepted, created_by, taken)."""
    s1, v1 = p["side1"], p["view1"]
    n1, K = len(s1["desc"]), len(p["side2"])
    taken0 = np.zeros(n1, np.uint8) if s1.get("has_lm") is None else np.asarray(s1["has_lm"], np.uint8).copy()
    taken = taken0.copy()
    out = dict(matched_2_in_1=np.full((K, n1), -1, np.int32), pos_w=np.zeros((K, n1, 3)), status=np.full((K, n1), T.SKIPPED, np.uint8),
               margin=np.full((K, n1), np.inf), branch=np.full((K, n1), T.NONE), num_matches=np.zeros(K, np.int32), num_accepted=np.zeros(K, np.int32),
               created_by=np.full(n1, -1, np.int32))
    for k in range(K):
        if p.get("active") is not None and not p["active"][k]:
            continue
        s2, v2 = p["side2"][k], p["neighbours"][k]
        if n1 == 0 or len(s2["desc"]) == 0:
            continue
        m, num = O.match_for_triangulation(p["lowe_ratio"], check_orientation, s1["desc"], s1["angle"], v1["octave"], v1["bearings"],
                                           taken if carry else taken0, s2["desc"], s2["angle"], v2["bearings"], s2.get("has_lm"), p["E_12"][k],
                                           p["epipole_in_2"][k], int(p["valid_epipole"][k]), p["tables"]["scale_factors"], p["residual_rad_thr"],
                                           xright1=v1.get("xright"), xright2=v2.get("xright"), node1=s1.get("node"), node2=s2.get("node"))
        r = T.restate_problem(dict(view1=v1, view2=v2, tables=p["tables"], idx1=m, idx2=None, deg_thr=p["deg_thr"]), null)
        out["matched_2_in_1"][k], out["num_matches"][k] = m, int(num)
        out["pos_w"][k], out["status"][k], out["margin"][k], out["branch"][k] = r["pos_w"], r["status"], r["margin"], r["branch"]
        acc = r["status"] == T.ACCEPTED
        out["num_accepted"][k] = int(acc.sum())
        out["created_by"][acc & (out["created_by"] < 0)] = k
        taken = taken | acc.astype(np.uint8)
    out["taken"] = taken
    return out


def permuted(p, order):
    """The same problem with its neighbours in another order."""
    order = list(order)
    q = dict(p)
    q["side2"], q["neighbours"] = [p["side2"][k] for k in order], [p["neighbours"][k] for k in order]
    for key in ("E_12", "epipole_in_2", "valid_epipole"):
        q[key] = np.ascontiguousarray(np.asarray(p[key])[order])
    if p.get("active") is not None:
        q["active"] = np.ascontiguousarray(p["active"][order])
    return q


# ------------------------------------------------------------------------------------------------ the device paths (GPU test, tools/bench_new_landmarks.py)
def device_view(v):
    from stella_vslam_amd.camera import svgpu_camera
    cam, c = v["cam"], svgpu_camera()
    c.model, c.cols, c.rows, c.fx, c.fy, c.cx, c.cy = cam["model"], cam["cols"], cam["rows"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    c.focal_x_baseline = cam["focal_x_baseline"]
    c.min_x, c.max_x, c.min_y, c.max_y = cam["bounds"]
    return dict(v, cam=c)


def run_device(ctx, p, ori=True):
    from stella_vslam_amd import match
    return match.new_landmarks_batch(ctx, p["lowe_ratio"], ori, p["side1"], device_view(p["view1"]), p["side2"], [device_view(v) for v in p["neighbours"]], p["E_12"],
                                     p["epipole_in_2"], p["valid_epipole"], p["tables"]["scale_factors"], p["tables"]["level_sigma_sq"],
                                     p["residual_rad_thr"], active=p.get("active"), rays_parallax_deg_thr=p["deg_thr"])


def single_device_calls(ctx, p, ori=True):
    """The only path that gave these results before: per neighbour one matcher call and one triangulator call, has_lm1 updated between them."""
    from stella_vslam_amd import match
    s1, v1 = p["side1"], p["view1"]
    n1, K = len(s1["desc"]), len(p["side2"])
    g1 = device_view(v1)
    taken = np.asarray(s1["has_lm"], np.uint8).copy()
    out = dict(matched_2_in_1=np.full((K, n1), -1, np.int32), pos_w=np.zeros((K, n1, 3)), status=np.full((K, n1), T.SKIPPED, np.uint8),
               num_matches=np.zeros(K, np.int32), num_accepted=np.zeros(K, np.int32), created_by=np.full(n1, -1, np.int32))
    for k in range(K):
        if p.get("active") is not None and not p["active"][k]:
            continue
        s2, v2 = p["side2"][k], p["neighbours"][k]
        m, num = match.match_for_triangulation(ctx, p["lowe_ratio"], ori, s1["desc"], s1["angle"], v1["octave"], v1["bearings"], taken, s2["desc"], s2["angle"],
                                               v2["bearings"], s2["has_lm"], p["E_12"][k], p["epipole_in_2"][k], int(p["valid_epipole"][k]),
                                               p["tables"]["scale_factors"], p["residual_rad_thr"], xright1=v1.get("xright"), xright2=v2.get("xright"),
                                               node1=s1.get("node"), node2=s2.get("node"))
        out["matched_2_in_1"][k], out["num_matches"][k] = m, num
        if n1 == 0:
            continue
        pos, st, acc = match.triangulate_two_views(ctx, g1, device_view(v2), p["tables"]["scale_factors"], p["tables"]["level_sigma_sq"], m, None, p["deg_thr"])
        out["pos_w"][k], out["status"][k], out["num_accepted"][k] = pos, st, acc
        got = st == T.ACCEPTED
        out["created_by"][got] = k
        taken = taken | got.astype(np.uint8)
    return out


def composed_batches(ctx, p, ori=True):
    """The two existing batch calls composed -- every neighbour under taken_0: NOT the loop's result where a keypoint matches in two neighbours."""
    from stella_vslam_amd import match
    k = len(p["side2"])
    lists, nums = match.match_for_triangulation_batch(ctx, p["lowe_ratio"], ori, dict(p["side1"], octave=p["view1"]["octave"], bearings=p["view1"]["bearings"],
                                                                                      xright=p["view1"].get("xright")),
                                                      [dict(s, bearings=v["bearings"], xright=v.get("xright")) for s, v in zip(p["side2"], p["neighbours"])],
                                                      p["E_12"], p["epipole_in_2"], p["valid_epipole"], p["tables"]["scale_factors"], p["residual_rad_thr"])
    off = np.arange(k + 1, dtype=np.int32) * len(p["side1"]["desc"])
    pos, st, acc = match.triangulate_two_views_batch(ctx, device_view(p["view1"]), [device_view(v) for v in p["neighbours"]], off,
                                                     p["tables"]["scale_factors"], p["tables"]["level_sigma_sq"], np.concatenate(lists), None, p["deg_thr"])
    return np.stack(lists), st.reshape(k, -1), nums, acc
