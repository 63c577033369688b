"""Problems for svgpu_fuse_landmarks_batch and a restatement of mapping_module::fuse_landmark_duplication (mapping_module.cc:417-537) on
flat arrays.  `chain` is written over three functions -- detect_duplication, compute_descriptor, update_geometry -- so the same text is the
CPU restatement (oracle.py's fuse and landmark-refresh restatements, as they are) and, on the device tests, the chain of single device
calls with the host update between them.  `carry=False` runs every pass on the snapshot instead: K independent calls.

A problem is a dict: keyframes (slot 0 = the current keyframe; each with cam parameters, pose, keypoints, kp_lm, observer), the observer
table, the landmark table with slack in its observation lists, the forward and backward lists and the ORB tables."""
import numpy as np

NONE, NEW_CONNECTION, DUP_SURVIVED, DUP_LOST, SAME_ID, SKIPPED = 0, 1, 2, 3, 4, 5
W, H, FX, CX, CY = 640, 480, 400.0, 320.0, 240.0
NUM_LEVELS, SCALE = 8, 1.2
STATE = ("alive", "descriptor", "mean_normal", "min_valid_dist", "max_valid_dist", "has_descriptor", "has_geometry", "obs_cnt", "obs_observer", "obs_kp",
         "obs_desc", "obs_weight")


def orb_tables():
    sf = np.cumprod(np.concatenate([[np.float32(1.0)], np.full(NUM_LEVELS - 1, np.float32(SCALE))]).astype(np.float32)).astype(np.float32)
    inv_sf = (np.float32(1.0) / sf).astype(np.float32)
    sigma = (sf * sf).astype(np.float32)
    return dict(scale_factors=sf, inv_level_sigma_sq=(np.float32(1.0) / sigma).astype(np.float32), log_scale_factor=float(np.float32(np.log(np.float32(SCALE)))),
                inv_scale_factor_last=float(inv_sf[-1]))


def _flip(rng, d, bits):
    out = d.copy()
    for b in rng.choice(256, bits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def project(model, pc):
    """camera::*::reproject_to_image for points in camera coordinates (fisheye reprojects as a pinhole: fisheye.cc:169-187)"""
    pc = np.asarray(pc, np.float64).reshape(-1, 3)
    if model == "equirectangular":
        b = pc / np.linalg.norm(pc, axis=1)[:, None]
        lat, lon = -np.arcsin(b[:, 1]), np.arctan2(b[:, 0], b[:, 2])
        return np.stack([W * (0.5 + lon / (2.0 * np.pi)), H * (0.5 - lat / np.pi)], 1)
    return np.stack([FX * pc[:, 0] / pc[:, 2] + CX, FX * pc[:, 1] / pc[:, 2] + CY], 1)


def build(name="basic", K=2, n_points=60, n_extra=2, n_clutter=40, stereo=False, reproj=True, model="perspective", seed=0, dup_frac=0.5, heavy_targets=False,
          empty_target=None, all_minus_one=False, crowd=0, same_id=0, conflict=False, slack=None, chain2=False):
    """K targets around the current keyframe.  Every 3-D point has a landmark A held by the current keyframe (and by `n_extra` keyframes that
    are no targets); a fraction `dup_frac` of the points also has a second landmark B held by the targets that see the point (the duplicates);
    the other points' keypoints in the targets hold no landmark (the new connections)."""
    rng = np.random.default_rng(seed)
    T = orb_tables()
    sf = T["scale_factors"]
    fxb = 40.0 if stereo else 0.0
    slots = K + 1
    O = slots + n_extra
    ids = rng.permutation(O * 3)[:O].astype(np.int32)  # keyframe ids: the rank of an observer, unrelated to its index
    centres = np.zeros((O, 3))
    centres[:, 0] = np.linspace(-0.25, 0.25, O)[rng.permutation(O)]
    centres[:, 1] = rng.uniform(-0.05, 0.05, O)
    pts = np.stack([rng.uniform(-2.0, 2.0, n_points), rng.uniform(-1.4, 1.4, n_points), rng.uniform(5.0, 9.0, n_points)], 1)
    base = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    p_oct = rng.integers(0, 3, n_points)
    kfs = []
    kp_of_point = []
    for u in range(slots):
        n_here = 0 if empty_target == u else n_points
        rel = pts[:n_here] - centres[u]
        xy = project(model, rel) + rng.uniform(-0.3, 0.3, (n_here, 2))
        desc = np.stack([_flip(rng, base[j], int(rng.integers(0, 12))) for j in range(n_here)]) if n_here else np.zeros((0, 32), np.uint8)
        octave = p_oct[:n_here].copy()
        nc = 0 if empty_target == u else n_clutter
        cxy = np.stack([rng.uniform(5, W - 5, nc), rng.uniform(5, H - 5, nc)], 1)
        if crowd and u == 1:  # `crowd` keypoints inside one grid cell, next to point 0's projection
            cxy = np.concatenate([cxy, xy[0] + rng.uniform(-2.0, 2.0, (crowd, 2))])
            nc += crowd
        cdesc = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
        if crowd and u == 1:
            for j in range(crowd):
                cdesc[n_clutter + j] = _flip(rng, base[0], 20 + (j % 25))
        coct = rng.integers(0, 4, nc)
        xy_all = np.concatenate([xy, cxy]).astype(np.float32)
        n = len(xy_all)
        xright = None
        if stereo:
            depth = np.concatenate([rel[:, 2], rng.uniform(5, 9, nc)])
            xright = (xy_all[:, 0] - np.float32(fxb) / depth.astype(np.float32)).astype(np.float32)
            xright[rng.uniform(0, 1, n) < 0.3] = -1.0
        R = np.eye(3)
        kfs.append(dict(model=model, fxb=fxb, rot_cw=R, trans_cw=-R @ centres[u], desc=np.concatenate([desc, cdesc]).astype(np.uint8), xy=xy_all,
                        octave=np.concatenate([octave, coct]).astype(np.int32), xright=xright, kp_lm=np.full(n, -1, np.int32), observer=u, grid_cols=64,
                        grid_rows=48))
        kp_of_point.append(np.arange(n_here))
    # landmarks: A_j = slot j (current keyframe + the extra observers); B_j = n_points + j for the duplicated points
    has_b = rng.uniform(0, 1, n_points) < dup_frac
    Lm = n_points + int(has_b.sum())
    b_slot = np.full(n_points, -1)
    b_slot[has_b] = n_points + np.arange(int(has_b.sum()))
    obs = [[] for _ in range(Lm)]   # (observer, kp)
    for j in range(n_points):
        obs[j].append((0, j))
        kfs[0]["kp_lm"][j] = j
        for x in range(n_extra):
            if rng.uniform() < 0.7:
                obs[j].append((slots + x, j))
        if has_b[j]:
            seen = [u for u in range(1, slots) if empty_target != u and (heavy_targets or rng.uniform() < 0.7)]
            if not seen:
                seen = [u for u in range(1, slots) if empty_target != u][:1]
            for u in seen:
                obs[b_slot[j]].append((u, j))
                kfs[u]["kp_lm"][j] = b_slot[j]
            if heavy_targets:  # B outweighs A: the swap of :442
                for x in range(n_extra):
                    if all(o != slots + x for o, _ in obs[b_slot[j]]):
                        obs[b_slot[j]].append((slots + x, 600 + j))
    pos_w = np.concatenate([pts, pts[has_b]])

    def desc_of(o, kp, j):  # (a keyframe that is no target shows the point's descriptor with its own six flipped bits)
        return kfs[o]["desc"][kp] if o < slots else _flip(np.random.default_rng(1000 * o + kp), base[j], 6)

    def weight_of(o, kp):
        return 2 if (o < slots and kfs[o]["xright"] is not None and kfs[o]["xright"][kp] >= 0) else 1
    passes = K + 1
    off, cap, cnt = np.zeros(Lm, np.int32), np.zeros(Lm, np.int32), np.zeros(Lm, np.int32)
    e_obs, e_kp, e_desc, e_w = [], [], [], []
    ref_twc, ref_sf = np.zeros((Lm, 3)), np.zeros(Lm, np.float32)
    point_of = np.concatenate([np.arange(n_points), np.flatnonzero(has_b)])
    for l in range(Lm):
        lst = sorted(obs[l], key=lambda t: ids[t[0]])
        off[l] = len(e_obs)
        cnt[l] = len(lst)
        cap[l] = len(lst) + (passes + 8 if slack is None else slack)
        for o, kp in lst:
            e_obs.append(o), e_kp.append(kp), e_desc.append(desc_of(o, kp, point_of[l])), e_w.append(weight_of(o, kp))
        for _ in range(cap[l] - cnt[l]):
            e_obs.append(-7), e_kp.append(-7), e_desc.append(np.zeros(32, np.uint8)), e_w.append(0)
        o0, kp0 = lst[0]
        ref_twc[l] = centres[o0]
        ref_sf[l] = sf[kfs[o0]["octave"][kp0]] if o0 < slots else sf[p_oct[point_of[l]]]
    table = dict(pos_w=pos_w, ref_trans_wc=ref_twc, ref_scale_factor=ref_sf, obs_off=off, obs_cap=cap, alive=np.ones(Lm, np.uint8),
                 descriptor=np.zeros((Lm, 32), np.uint8), mean_normal=np.zeros((Lm, 3)), min_valid_dist=np.zeros(Lm, np.float32),
                 max_valid_dist=np.zeros(Lm, np.float32), has_descriptor=np.ones(Lm, np.uint8), has_geometry=np.ones(Lm, np.uint8), obs_cnt=cnt,
                 obs_observer=np.array(e_obs, np.int32), obs_kp=np.array(e_kp, np.int32), obs_desc=np.array(e_desc, np.uint8).reshape(-1, 32),
                 obs_weight=np.array(e_w, np.int32))
    p = dict(name=name, keyframes=kfs, observer_rank=ids, observer_trans_wc=centres, table=table, margin=3.0, do_reprojection_matching=reproj, **T)
    p["fwd_list"] = np.full(len(kfs[0]["kp_lm"]), -1, np.int32) if all_minus_one else kfs[0]["kp_lm"].copy()
    seen_b, bwd = set(), []
    for u in range(1, slots):
        for l in kfs[u]["kp_lm"]:
            if l >= 0 and l not in seen_b:
                seen_b.add(int(l)), bwd.append(int(l))
    p["bwd_list"] = np.array(bwd, np.int32)   # first appearance: target order, then keypoint order
    # plantings that make kp_lm and the observation lists disagree (the cases the reference meets only with a keyframe whose landmark vector
    # is ahead of its landmarks' observations)
    if same_id:  # the keypoint in target 1 already names the checked landmark, which has no observation there
        for j in np.flatnonzero(~has_b)[:same_id]:
            kfs[1]["kp_lm"][j] = j
    if conflict:  # the landmark a target keypoint holds is itself a checked landmark that hits in the same target
        free = np.flatnonzero(~has_b)
        a = max(int(j) for j in free if len(obs[j]) == 1 + n_extra)  # seen by every extra keyframe: it survives every comparison (:442)
        free = free[free < a]
        c = int(free[-1])
        kfs[1]["kp_lm"][a] = c     # A_a hits keypoint a, which holds A_c; A_c hits its own keypoint c (a new connection) in the same target
        if chain2:
            b = int(free[-2])
            kfs[1]["kp_lm"][c] = b  # ... and A_c's keypoint holds A_b: a replaced_by chain of length 2 in front of A_b's own connection
    return p


def initial_refresh(p, compute_descriptor, update_geometry):
    """The stored descriptor, mean normal and distance limits of every landmark from its initial list (the flags are up on entry)."""
    t = p["table"]
    Lm = len(t["obs_off"])
    coff = np.concatenate([[0], np.cumsum(t["obs_cnt"])]).astype(np.int32)
    sel = np.concatenate([np.arange(t["obs_off"][l], t["obs_off"][l] + t["obs_cnt"][l]) for l in range(Lm)]).astype(np.int64)
    _, t["descriptor"] = compute_descriptor(coff, t["obs_desc"][sel])
    t["mean_normal"], t["max_valid_dist"], t["min_valid_dist"] = update_geometry(coff, p["observer_trans_wc"][t["obs_observer"][sel]], t["pos_w"],
                                                                                t["ref_trans_wc"], t["ref_scale_factor"], p["inv_scale_factor_last"])
    return p


class Overflow(Exception):
    pass


def chain(p, cams, detect, compute_descriptor, update_geometry, carry=True, count=None):
    """fuse_landmark_duplication on the flat problem.  cams[u]: the camera of slot u in the type `detect` takes.  Returns the outputs of
    svgpu_fuse_landmarks_batch; raises Overflow when an observation list would outgrow its capacity."""
    t = {k: np.array(v, copy=True) for k, v in p["table"].items()}
    kfs = p["keyframes"]
    K = len(kfs) - 1
    kp_lm = [np.array(f["kp_lm"], copy=True) for f in kfs]
    rank, twc = p["observer_rank"], np.asarray(p["observer_trans_wc"], np.float64)
    Lm = len(t["obs_off"])
    observer_kf = {f["observer"]: u for u, f in enumerate(kfs)}
    replaced_by = np.full(Lm, -1, np.int32)
    snap = {k: v.copy() for k, v in t.items()} if not carry else None
    n_fwd, n_bwd = len(p["fwd_list"]), len(p["bwd_list"])
    best_all = np.full(K * n_fwd + n_bwd, -1, np.int32)
    event_all = np.zeros(K * n_fwd + n_bwd, np.uint8)
    num_fused = np.zeros(K + 1, np.int32)
    totals = np.zeros(K + 1, np.int64)

    def entries(l):
        return np.arange(t["obs_off"][l], t["obs_off"][l] + t["obs_cnt"][l])

    def find(l, o):
        e = entries(l)
        hit = np.flatnonzero(t["obs_observer"][e] == o)
        return int(e[hit[0]]) if len(hit) else -1

    def nobs(l):
        return int(t["obs_weight"][entries(l)].sum())

    def insert(l, o, kp, d, w):
        if t["obs_cnt"][l] >= t["obs_cap"][l]:
            raise Overflow()
        off, cnt = t["obs_off"][l], t["obs_cnt"][l]
        pos = cnt
        while pos > 0 and rank[t["obs_observer"][off + pos - 1]] > rank[o]:
            for k in ("obs_observer", "obs_kp", "obs_desc", "obs_weight"):
                t[k][off + pos] = t[k][off + pos - 1]
            pos -= 1
        t["obs_observer"][off + pos], t["obs_kp"][off + pos], t["obs_desc"][off + pos], t["obs_weight"][off + pos] = o, kp, d, w
        t["obs_cnt"][l] = cnt + 1
        t["has_descriptor"][l] = t["has_geometry"][l] = 0

    def refresh_desc(l):
        e = entries(l)
        _, d = compute_descriptor(np.array([0, len(e)], np.int32), t["obs_desc"][e])
        t["descriptor"][l] = d[0]
        t["has_descriptor"][l] = 1

    def refresh_geom(l):
        e = entries(l)
        mn, mx, mi = update_geometry(np.array([0, len(e)], np.int32), twc[t["obs_observer"][e]], t["pos_w"][l:l + 1], t["ref_trans_wc"][l:l + 1],
                                     t["ref_scale_factor"][l:l + 1], p["inv_scale_factor_last"])
        t["mean_normal"][l], t["max_valid_dist"][l], t["min_valid_dist"][l] = mn[0], mx[0], mi[0]
        t["has_geometry"][l] = 1

    for ps in range(K + 1):
        u = ps + 1 if ps < K else 0
        lst = np.asarray(p["fwd_list"] if ps < K else p["bwd_list"], np.int32)
        f = kfs[u]
        o_u = f["observer"]
        out0 = ps * n_fwd if ps < K else K * n_fwd
        if len(lst) == 0 or len(f["xy"]) == 0 or Lm == 0:
            continue
        s = snap if snap is not None else t
        idx = np.where(lst >= 0, lst, 0)
        if snap is not None:
            observed = np.array([l >= 0 and o_u in snap["obs_observer"][snap["obs_off"][l]:snap["obs_off"][l] + snap["obs_cnt"][l]] for l in lst])
        else:
            observed = np.array([l >= 0 and find(l, o_u) >= 0 for l in lst])
        valid = ((lst >= 0) & (s["alive"][idx] != 0) & ~observed).astype(np.uint8)
        best, num = detect(cams[u], f["rot_cw"], f["trans_cw"], s["pos_w"][idx], valid, s["min_valid_dist"][idx], s["max_valid_dist"][idx], s["mean_normal"][idx],
                           s["descriptor"][idx], p["scale_factors"], p["inv_level_sigma_sq"], p["log_scale_factor"], p["margin"], f["desc"], f["xy"], f["octave"],
                           t_xright=f["xright"], do_reprojection_matching=p["do_reprojection_matching"], grid_cols=f["grid_cols"], grid_rows=f["grid_rows"])
        best = np.asarray(best, np.int32)
        if count is not None:
            totals[ps] = count(p, cams[u], f, s["pos_w"][idx], valid, s["min_valid_dist"][idx], s["max_valid_dist"][idx], s["mean_normal"][idx])
        best_all[out0:out0 + len(lst)] = best
        num_fused[ps] = int((best >= 0).sum())
        if snap is not None:
            continue
        hit = np.full(len(lst), -1, np.int64)
        for i in np.flatnonzero(best >= 0):
            B = kp_lm[u][best[i]]
            hit[i] = -2 if B < 0 else (B if t["alive"][B] else -3)
        for i in np.flatnonzero(hit >= 0):   # :436-456, ascending list index
            A, B = int(lst[i]), int(hit[i])
            if A == B:
                event_all[out0 + i] = SAME_ID
                continue
            if not t["alive"][A] or not t["alive"][B]:
                event_all[out0 + i] = SKIPPED
                continue
            S, X = (B, A) if nobs(A) < nobs(B) else (A, B)
            event_all[out0 + i] = DUP_SURVIVED if S == A else DUP_LOST
            for e in entries(X):
                o, kp = int(t["obs_observer"][e]), int(t["obs_kp"][e])
                if o in observer_kf:
                    kp_lm[observer_kf[o]][kp] = -1
                if find(S, o) >= 0:
                    continue
                insert(S, o, kp, t["obs_desc"][e].copy(), int(t["obs_weight"][e]))
                if o in observer_kf:
                    kp_lm[observer_kf[o]][kp] = S
            t["alive"][X] = 0
            t["obs_cnt"][X] = 0
            replaced_by[X] = S
            if not t["has_descriptor"][S]:
                refresh_desc(S)
            if not t["has_geometry"][S]:
                refresh_geom(S)
        for i in np.flatnonzero(hit == -2):  # :458-467
            S = int(lst[i])
            while replaced_by[S] >= 0:
                S = int(replaced_by[S])
            b = int(best[i])
            w = 2 if (f["xright"] is not None and f["xright"][b] >= 0) else 1
            event_all[out0 + i] = NEW_CONNECTION
            kp_lm[u][b] = S
            e = find(S, o_u)
            if e >= 0:
                t["obs_kp"][e], t["obs_desc"][e] = b, f["desc"][b]
                t["obs_weight"][e] += w
                t["has_descriptor"][S] = t["has_geometry"][S] = 0
            else:
                insert(S, o_u, b, f["desc"][b].copy(), w)
            refresh_geom(S)
            refresh_desc(S)
    out = {k: t[k] for k in STATE}
    out.update(kp_lm=kp_lm, replaced_by=replaced_by, best_idx=best_all, event=event_all, num_fused=num_fused, cand_totals=totals)
    return out


def live_view(p, out):
    """What a caller can observe of a result: dead lists and the slack of live ones hold no information (the device leaves shifted copies there)."""
    t = p["table"]
    v = {k: np.array(out[k], copy=True) for k in ("alive", "replaced_by", "best_idx", "event", "num_fused", "obs_cnt", "has_descriptor", "has_geometry")}
    v["kp_lm"] = np.concatenate([np.asarray(a) for a in out["kp_lm"]]) if len(out["kp_lm"]) else np.zeros(0, np.int32)
    live = np.flatnonzero(np.asarray(out["alive"]) != 0)
    for k in ("descriptor", "mean_normal", "min_valid_dist", "max_valid_dist"):
        v[k] = np.asarray(out[k])[live].copy()
    sel = np.concatenate([np.arange(t["obs_off"][l], t["obs_off"][l] + out["obs_cnt"][l]) for l in live] + [np.zeros(0, np.int64)]).astype(np.int64)
    for k in ("obs_observer", "obs_kp", "obs_desc", "obs_weight"):
        v[k] = np.asarray(out[k])[sel].copy()
    return v


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(p, a, b, what=""):
    va, vb = live_view(p, a), live_view(p, b)
    for k in va:
        assert va[k].shape == vb[k].shape and np.array_equal(bits(va[k]), bits(vb[k])), (p["name"], what, k)


def count_candidates(p, cam, f, pos_w, valid, min_d, max_d, normal):
    """The candidate-list total of one pass (fuse.cc:37-74 in numpy, the lists by the oracle's get_keypoints_in_cell): what the device's arena holds."""
    from oracle import oracle as O
    R, t = np.asarray(f["rot_cw"], np.float64), np.asarray(f["trans_cw"], np.float64)
    pc = pos_w @ R.T + t
    ok = valid > 0
    if f["model"] != "equirectangular":
        ok &= pc[:, 2] > 0
    uv = project(f["model"], np.where(ok[:, None], pc, [0.0, 0.0, 1.0]))
    if f["model"] == "radial_division":
        ok &= ~((uv[:, 0] < cam.min_x) | (uv[:, 0] > cam.max_x)) & ~((uv[:, 1] < cam.min_y) | (uv[:, 1] > cam.max_y))
    elif f["model"] != "equirectangular":
        ok &= (cam.min_x < uv[:, 0]) & (uv[:, 0] < cam.max_x) & (cam.min_y < uv[:, 1]) & (uv[:, 1] < cam.max_y)
    v = pos_w - (-R.T @ t)
    dist = np.linalg.norm(v, axis=1)
    ok &= ~((dist < (1.0 / 1.3) * min_d.astype(np.float64)) | (1.3 * max_d.astype(np.float64) < dist))
    ok &= ~((v * normal).sum(1) < 0.5 * dist)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (max_d / dist.astype(np.float32)).astype(np.float32)
        lv = np.ceil(np.log(ratio.astype(np.float64)).astype(np.float32) / np.float32(p["log_scale_factor"]))
    lv = np.clip(np.where(ok, lv, 0), 0, NUM_LEVELS - 1).astype(int)
    qm = (np.float32(p["margin"]) * p["scale_factors"][lv]).astype(np.float32)
    bounds = (cam.min_x, cam.max_x, cam.min_y, cam.max_y)
    kx, ky = np.ascontiguousarray(f["xy"][:, 0]), np.ascontiguousarray(f["xy"][:, 1])
    off, items = O.assign_keypoints_to_grid(kx, ky, bounds, f["grid_cols"], f["grid_rows"])
    total = 0
    for q in np.flatnonzero(ok):
        total += len(O.get_keypoints_in_cell(kx, ky, f["octave"], off, items, bounds, np.float32(uv[q, 0]), np.float32(uv[q, 1]), np.float32(qm[q]),
                                             int(max(0, lv[q] - 1)), int(min(NUM_LEVELS - 1, lv[q] + 1))))
    return total


def _flip_bits(d, lo, hi):
    out = d.copy()
    for b in range(lo, hi):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def planted(name, seed=0):
    """Classes whose carry is constructed bit by bit.  Two targets, no duplicates: every checked landmark connects at target 1.
    desc_flip      target 1 ranks in front of the current keyframe, so the refreshed descriptor (two observations: the first in map order wins)
                   is target 1's keypoint, 30 bits from the stored one; the keypoint in target 2 is 30 OTHER bits from the stored descriptor and
                   60 from the refreshed one: the snapshot matches it, the chain does not.
    level_move     the stored limits are stale (max_valid_dist = the distance itself: level 0) while the reference keypoint's scale factor is the
                   top level's: the refresh behind the connection at target 1 moves the predicted level to 7 and the window to levels 6..7 and
                   3 * 1.2^7 pixels; target 2 holds, beside the point's own level-0 keypoint, `m` level-6 keypoints that match: the snapshot
                   takes the own keypoint, the chain a level-6 one.  arena_overflow is the same with m = 40: the lists of the pass into
                   target 2 outgrow the arena sized from the snapshot."""
    from oracle import oracle as O
    n_pts = 60
    p = build(name=name, K=2, n_points=n_pts, n_extra=0, dup_frac=0.0, n_clutter=(20 if name == "desc_flip" else 0), seed=seed + sum(map(ord, name)))
    kfs, t = p["keyframes"], p["table"]
    if name == "desc_flip":
        p["observer_rank"] = np.array([5, 2, 9], np.int32)
        for j in range(n_pts):
            kfs[1]["desc"][j] = _flip_bits(kfs[0]["desc"][j], 0, 30)
            kfs[2]["desc"][j] = _flip_bits(kfs[0]["desc"][j], 100, 130)
        return initial_refresh(p, O.landmarks_compute_descriptor, O.landmarks_update_geometry)
    m = 40 if name == "arena_overflow" else 2
    rng = np.random.default_rng(seed + 17)
    for f in kfs:
        f["octave"][:n_pts] = 0
    f2 = kfs[2]
    xy = np.repeat(f2["xy"][:n_pts], m, 0) + rng.uniform(-3.0, 3.0, (n_pts * m, 2)).astype(np.float32)
    desc = np.stack([_flip(rng, kfs[0]["desc"][j], 4) for j in range(n_pts) for _ in range(m)])
    f2["xy"] = np.concatenate([f2["xy"], xy]).astype(np.float32)
    f2["desc"] = np.concatenate([f2["desc"], desc]).astype(np.uint8)
    f2["octave"] = np.concatenate([f2["octave"], np.full(n_pts * m, 6, np.int32)]).astype(np.int32)
    f2["kp_lm"] = np.concatenate([f2["kp_lm"], np.full(n_pts * m, -1, np.int32)]).astype(np.int32)
    t["ref_scale_factor"] = np.ones_like(t["ref_scale_factor"])
    initial_refresh(p, O.landmarks_compute_descriptor, O.landmarks_update_geometry)  # the stale limits: as if the reference keypoint were level 0
    t["ref_scale_factor"] = np.full_like(t["ref_scale_factor"], p["scale_factors"][7])
    return p


PLANTED = ("desc_flip", "level_move")

CLASSES = dict(
    k1=dict(K=1), basic=dict(K=2), k4=dict(K=4, n_points=80), k12=dict(K=12, n_points=40, n_clutter=24), stereo=dict(K=2, stereo=True),
    no_reproj=dict(K=2, reproj=False), radial=dict(K=2, model="radial_division"), fisheye=dict(K=2, model="fisheye"),
    equirectangular=dict(K=2, model="equirectangular"), swap=dict(K=2, heavy_targets=True), empty_target=dict(K=2, empty_target=1),
    all_minus_one=dict(K=2, all_minus_one=True), cell64=dict(K=2, crowd=63), cell65=dict(K=2, crowd=64), same_id=dict(K=2, same_id=3),
    conflict=dict(K=2, conflict=True), chain2=dict(K=2, conflict=True, chain2=True), cap_exact=dict(K=1, dup_frac=1.0, heavy_targets=False, n_extra=0, slack=1),
)
OVERFLOW = dict(K=1, dup_frac=1.0, n_extra=0, slack=0)


def make(name, seed=0):
    kw = OVERFLOW if name == "overflow" else CLASSES[name]
    return build(name=name, seed=seed + sum(map(ord, name)), **kw)


def oracle_cams(p):
    from oracle import oracle as O
    out = []
    for f in p["keyframes"]:
        model = dict(perspective=O.CAM_PERSPECTIVE, fisheye=O.CAM_FISHEYE, equirectangular=O.CAM_EQUIRECTANGULAR, radial_division=O.CAM_RADIAL_DIVISION)[f["model"]]
        dist = dict(perspective=(0, 0, 0, 0, 0), fisheye=(0, 0, 0, 0), equirectangular=(), radial_division=(0.0,))[f["model"]]
        out.append(O.make_camera(model, W, H, FX, FX, CX, CY, dist, f["fxb"]))
    return out


def cpu_chain(p, carry=True):
    from oracle import oracle as O
    return chain(p, oracle_cams(p), O.fuse_detect_duplication, O.landmarks_compute_descriptor, O.landmarks_update_geometry, carry=carry,
                 count=count_candidates)


def prepared(name, seed=0):
    from oracle import oracle as O
    if name in PLANTED or name == "arena_overflow":
        return planted(name, seed)
    return initial_refresh(make(name, seed), O.landmarks_compute_descriptor, O.landmarks_update_geometry)


ALL = list(CLASSES) + list(PLANTED)
CAND_FACTOR, CAND_SLACK = 2, 1024   # fuse_layout.h: FUSE_CAND_FACTOR, FUSE_CAND_SLACK


def cand_capacity(p):
    """fuse_cand_capacity of the snapshot totals"""
    return CAND_FACTOR * int(cpu_chain(p, carry=False)["cand_totals"].max(initial=0)) + CAND_SLACK
