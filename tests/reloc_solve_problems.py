"""Problems for svgpu_reloc_solve_batch (PnP -> pose optimisation -> bookkeeping -> refine_pose for all candidates in one call) and the
yardstick `chain`: the same steps one candidate at a time over a PnP solver, a pose optimiser and a one-candidate refine_pose given as
callables (the device's single calls in tests/test_gpu_reloc_solve.py, the CPU restatements in tests/test_reloc_solve_problem_classes.py),
with the host steps of module/relocalizer.cc:103-123 between them written in numpy.

The scenes are those of tests/reloc_refine_problems.py (one frame, K candidates over one set of landmarks): what that builder calls "the
frame's landmarks after optimize_pose" are here the candidate's 2D-3D matches in front of PnP -- keypoint-index order, the n_bad of them
with a position 0.8 m off (outliers of PnP).  m_kf_entry is found by position: a match whose landmark is one of the candidate's keyframe
entries names it (and the entry is offered, valid = 1: the call itself spends it), a wrong position names none (-1, a neighbour's).
Sample tables come from tests/pnp_problems.draw_samples, the helper of the PnP tests.

n_shifted: that many of the offered entries get a position 5 px x scale of their level sideways, alternating in sign: the first stage
(window 10 px x scale) matches them and the optimisation rejects them (> 4 sigma) -- matches that pass a count test and are not valid
behind it.

Which status values scenes can reach: with ONE threshold for optimize_pose and refine_pose the first stage's count test could never fail
(n_already_found is the count optimize_pose just passed), which is why the optimise step has its own threshold as in the reference
(min_num_bow_matches_ / 2, relocalizer.cc:220).  The final failure of a TWO-stage chain needs matches that only the second stage's
narrower window finds; from a PnP pose over exact matches there are none, so that value is reached with one stage only (status 1 + 1)."""
import numpy as np

from oracle import oracle as O
from tests import pnp_problems as PP
from tests import reloc_refine_problems as RP

PNP_FAILED, OPTIMIZE_FAILED = -2, -3
NUM_ITER = 12
MIN_INLIERS = 10
MIN_OPT = 25  # min_num_opt_valid_obs of the classes


def camera(problem):
    c = problem["cam"]
    return O.make_camera(c["model"], c["cols"], c["rows"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"], c["focal_x_baseline"])


def make(name, cands, shifted=None, seed=1, **kw):
    """RP.make's problem turned into the solve call's: match_off / m_keypt / m_pos_w / m_kf_entry / samples / t_bearings added, the
    per-candidate state of the refine call (pose_cw, n_already_found, frame_has_lm, frame_lm_pos_w) dropped."""
    p = RP.make(name, cands, seed=seed, **kw)
    K, off = p["num_candidates"], p["kf_off"]
    shifted = shifted or [0] * K
    sf = p["scale_factors"]
    moff, keypt, mpos, ment, samples = [0], [], [], [], []
    valid, pos_w = p["valid"].copy(), p["pos_w"].copy()
    for c in range(K):
        lo, hi = int(off[c]), int(off[c + 1])
        kp = np.flatnonzero(p["frame_has_lm"][c]).astype(np.int32)
        pos = p["frame_lm_pos_w"][c][kp]
        ent = np.full(len(kp), -1, np.int32)
        for i, x in enumerate(pos):
            hit = np.flatnonzero((p["pos_w"][lo:hi] == x).all(1))
            if len(hit):
                ent[i] = hit[0]
                valid[lo + hit[0]] = 1
        # (n_shifted) offered entries that no match names: sideways along the camera's x axis (the scene's rotation is within 1.3 degrees of
        # the identity), by 5 px x scale of the level the matcher predicts for the entry
        free = [i for i in np.flatnonzero(p["valid"][lo:hi]) if i not in set(ent.tolist())][:shifted[c]]
        for j, i in enumerate(free):
            z = pos_w[lo + i, 2] + 0.1
            level = int(round(np.log(p["max_valid_dist"][lo + i] / (0.9 * np.linalg.norm(pos_w[lo + i]))) / np.log(1.2)))
            pos_w[lo + i, 0] += (1.0 if j % 2 == 0 else -1.0) * 5.0 * float(sf[np.clip(level, 0, len(sf) - 1)]) * z / RP.FX
        keypt.append(kp), mpos.append(pos), ment.append(ent)
        moff.append(moff[-1] + len(kp))
        samples.append(PP.draw_samples(np.random.default_rng(7000 + 31 * seed + c), len(kp), NUM_ITER))
    q = {k: v for k, v in p.items() if k not in ("pose_cw", "n_already_found", "frame_has_lm", "frame_lm_pos_w")}
    q.update(valid=valid, pos_w=pos_w, t_bearings=O.keypoints_to_bearings(camera(p), p["t_xy"]), match_off=np.array(moff, np.int32),
             m_keypt=np.concatenate(keypt).astype(np.int32), m_pos_w=np.ascontiguousarray(np.concatenate(mpos), np.float64).reshape(-1, 3),
             m_kf_entry=np.concatenate(ment).astype(np.int32), samples=np.stack(samples).astype(np.uint32), min_num_inliers=MIN_INLIERS,
             num_iter=NUM_ITER, recompute=0, gauss_newton_num_iter=10, min_num_opt_valid_obs=MIN_OPT)
    return q


ACCEPT = lambda seed=0, **kw: RP.cand(n_init=60, n_bad=8, n_entries=300, seed=seed, **kw)   # ~52 inliers, ~150 matches in the first stage
FEW = RP.cand(n_init=8, n_entries=200)                         # fewer than min_num_inliers matches: PnP launches nothing
GARBAGE = RP.cand(n_init=40, n_bad=40, n_entries=200)          # no hypothesis with more than 10 inliers
THIN = RP.cand(n_init=23, n_bad=2, n_entries=300)              # PnP valid on 21 inliers, optimize_pose below its 25
FIRST = RP.cand(n_init=34, n_bad=3, n_entries=150, n_valid=8)  # 31 + at most 8 found < 50: status 1
SECOND = RP.cand(n_init=34, n_bad=3, n_entries=300, n_valid=80)  # (with 80 shifted) 31 + the shifted matches pass, 31 stay valid: status 2
NO_ENTRIES = RP.cand(n_init=70, n_bad=5, n_entries=0)          # an empty keyframe list: accepted on its PnP inliers


def classes():
    P = {}
    P["accepted"] = make("accepted", [ACCEPT(1), ACCEPT(2), ACCEPT(3), ACCEPT(4), ACCEPT(5)], seed=21)
    P["each_status"] = make("each_status", [ACCEPT(1), FEW, GARBAGE, THIN, FIRST, SECOND, ACCEPT(2, active=0)], shifted=[0, 0, 0, 0, 0, 80, 0], seed=22)
    P["one_stage"] = make("one_stage", [ACCEPT(1), SECOND, FIRST], shifted=[0, 80, 0], num_stages=1, seed=23)
    P["stereo"] = make("stereo", [ACCEPT(1), THIN, ACCEPT(2)], stereo=True, seed=24)
    P["degenerate"] = make("degenerate", [NO_ENTRIES, RP.cand(n_init=0, n_entries=200), RP.cand(n_init=3, n_entries=200), ACCEPT(1)], seed=25)
    return P


EXPECT = dict(accepted=[0] * 5, each_status=[0, PNP_FAILED, PNP_FAILED, OPTIMIZE_FAILED, 1, 2, -1], one_stage=[0, 2, 1],
              stereo=[0, OPTIMIZE_FAILED, 0], degenerate=[0, PNP_FAILED, PNP_FAILED, 0])

PER_CAND = ("status", "pnp_valid", "pnp_pose_cw", "best_iter", "opt_pose", "opt_num_valid", "pose_out", "outlier", "num_found", "num_valid", "lm_iterations")
PER_MATCH = ("is_inlier", "opt_outlier")
PER_ENTRY = ("match_kf", "match_stage")
OUTPUTS = PER_CAND + PER_MATCH + PER_ENTRY


def sub(problem, keep):
    """the problem with the candidates `keep` (indices, in that order) alone"""
    keep = list(keep)
    q = RP.sub(dict(problem, pose_cw=np.zeros((problem["num_candidates"], 12)), n_already_found=np.zeros(problem["num_candidates"], np.int32),
                    frame_has_lm=np.zeros((problem["num_candidates"], 1), np.uint8), frame_lm_pos_w=np.zeros((problem["num_candidates"], 1, 3))), keep)
    for k in ("pose_cw", "n_already_found", "frame_has_lm", "frame_lm_pos_w"):
        del q[k]
    rows = match_rows(problem, keep)
    for k in ("m_keypt", "m_pos_w", "m_kf_entry"):
        q[k] = np.ascontiguousarray(problem[k][rows])
    mo = problem["match_off"]
    q["match_off"] = np.concatenate([[0], np.cumsum([mo[p + 1] - mo[p] for p in keep])]).astype(np.int32)
    q["samples"] = np.ascontiguousarray(problem["samples"][keep]) if keep else np.zeros((0, problem["num_iter"], 4), np.uint32)
    return q


def match_rows(problem, keep):
    mo = problem["match_off"]
    return np.concatenate([np.arange(mo[p], mo[p + 1]) for p in keep]).astype(np.int64) if len(keep) else np.zeros(0, np.int64)


def chain(problem, backend, **over):
    """reloc_by_candidate behind the BoW matcher per candidate, as the host loop.  backend = (pnp(problem, bearings, pos_w, octaves, samples)
    -> (valid, pose12, is_inlier, best_iter), optimize(problem, pose, pos_w, uvr, w, huber) -> (num_valid, pose, flags, lm_iterations),
    refine(one-candidate refine problem) -> the dict of refine_pose_batch)."""
    do_pnp, do_opt, do_refine = backend
    p = dict(problem, **over)
    K, S, nt = p["num_candidates"], p["num_stages"], p["nt"]
    off, mo = p["kf_off"], p["match_off"]
    N, M = int(off[-1]), int(mo[-1])
    out = dict(status=np.zeros(K, np.int32), pnp_valid=np.zeros(K, np.uint8), pnp_pose_cw=np.zeros((K, 12)), is_inlier=np.zeros(M, np.uint8),
               best_iter=np.full(K, -1, np.int32), opt_pose=np.zeros((K, 12)), opt_outlier=np.zeros(M, np.uint8), opt_num_valid=np.zeros(K, np.int32),
               pose_out=np.zeros((K, 12)), match_kf=np.full(N, -1, np.int32), match_stage=np.full(N, -1, np.int32), outlier=np.zeros((K, nt), np.uint8),
               num_found=np.zeros((K, S), np.int32), num_valid=np.zeros((K, S), np.int32), lm_iterations=np.zeros(K, np.int32))
    xr = p["t_xright"]
    uvr_all = np.concatenate([p["t_xy"], (np.full(nt, -1, np.float32) if xr is None else xr)[:, None]], 1).astype(np.float32)
    w_all = p["inv_level_sigma_sq"][p["t_octave"]].astype(np.float32)
    hb = RP.huber_delta(p)
    for c in range(K):
        if p["active"] is not None and not p["active"][c]:
            out["status"][c] = -1
            continue
        lo, hi = int(mo[c]), int(mo[c + 1])
        kp, pos, ent = p["m_keypt"][lo:hi], p["m_pos_w"][lo:hi], p["m_kf_entry"][lo:hi]
        # 1. PnP (relocalizer.cc:191-197)
        valid, pose, inl, best = do_pnp(p, p["t_bearings"][kp], pos, p["t_octave"][kp], p["samples"][c])
        out["pnp_valid"][c], out["best_iter"][c] = valid, best
        out["pnp_pose_cw"][c] = out["opt_pose"][c] = out["pose_out"][c] = np.asarray(pose, np.float64).reshape(12)
        out["is_inlier"][lo:hi] = inl
        if not valid:
            out["status"][c] = PNP_FAILED
            continue
        # 2. optimize_pose over the inliers, in entry order (:104-108, :211-234)
        sel = np.flatnonzero(inl)
        nv, pose2, flags, _ = do_opt(p, out["pnp_pose_cw"][c], pos[sel], uvr_all[kp[sel]], w_all[kp[sel]], np.full(len(sel), hb, np.float32))
        out["opt_pose"][c] = out["pose_out"][c] = np.asarray(pose2, np.float64).reshape(12)
        out["opt_outlier"][lo + sel] = np.asarray(flags, np.uint8)[:len(sel)]
        out["opt_num_valid"][c] = nv
        if nv < p["min_num_opt_valid_obs"]:
            out["status"][c] = OPTIMIZE_FAILED
            continue
        # 3. the bookkeeping (:116-123 and the outlier erasure of optimize_pose)
        held = np.flatnonzero((np.asarray(inl) != 0) & (out["opt_outlier"][lo:hi] == 0))
        has, lm_pos = np.zeros((1, nt), np.uint8), np.zeros((1, nt, 3))
        has[0, kp[held]] = 1
        lm_pos[0, kp[held]] = pos[held]
        r0, r1 = int(off[c]), int(off[c + 1])
        kf_valid = p["valid"][r0:r1].copy()
        kf_valid[ent[held][ent[held] >= 0]] = 0
        # 4. refine_pose, one candidate
        one = {k: v for k, v in p.items()}
        one.update(num_candidates=1, active=None, pose_cw=out["opt_pose"][c:c + 1].copy(), n_already_found=np.array([len(held)], np.int32), frame_has_lm=has,
                   frame_lm_pos_w=lm_pos, kf_off=np.array([0, r1 - r0], np.int32), valid=kf_valid)
        for k in ("pos_w", "min_valid_dist", "max_valid_dist", "lm_desc", "angle_kf"):
            one[k] = np.ascontiguousarray(p[k][r0:r1])
        r = do_refine(one)
        for k in ("status", "pose_out", "outlier", "num_found", "num_valid", "lm_iterations"):
            out[k][c] = r[k][0]
        out["match_kf"][r0:r1], out["match_stage"][r0:r1] = r["match_kf"], r["match_stage"]
    return out


def same(a, b, keys=OUTPUTS):
    """every output element for element, the poses as raw 64-bit patterns; returns the names that differ"""
    return [k for k in keys if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes() or np.shape(a[k]) != np.shape(b[k])]
