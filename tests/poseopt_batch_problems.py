"""Problems for svgpu_pose_optimize_batch, one per class of input the batch kernel treats differently.  Every class states the property that
makes it a class; tests/test_poseopt_batch_problem_classes.py holds each to it under the CPU oracle, tests/test_gpu_poseopt_batch.py runs them
all in one batch per camera (the intrinsics are shared per call).  The observations come from tests.test_oracle_ba._pose_problem and
synthetic.ba_scene, sliced to exact sizes."""
import functools

import numpy as np

from stella_vslam_amd import synthetic as S
from tests.test_oracle_ba import _pose_problem

# wave (64) and workgroup-stride (512) boundaries of k_pose_opt_batch, the skip threshold (5), and a size of several strides
SIZES = (0, 4, 5, 63, 64, 65, 511, 512, 513, 1200)


def _problem(name, prop, src, n, select=None, active=True):
    assert len(src["pos_w"]) >= n, (name, len(src["pos_w"]), n)
    p = dict(name=name, property=prop, pose_cw=np.ascontiguousarray(src["pose_cw"], np.float64).reshape(12),
             pos_w=np.ascontiguousarray(src["pos_w"][:n], np.float64), uvr=np.ascontiguousarray(src["uvr"][:n], np.float32),
             inv_sigma_sq=np.ascontiguousarray(src["inv_sigma_sq"][:n], np.float32), huber=np.ascontiguousarray(src["huber"][:n], np.float32),
             intr=np.ascontiguousarray(src["intr"], np.float64).reshape(5), select=None if select is None else np.ascontiguousarray(select, np.uint8),
             active=bool(active))
    assert p["select"] is None or len(p["select"]) == n
    return p


def _equirect_source(seed, n):
    sc = S.ba_scene(num_kf=3, num_lm=n, obs_per_lm=3, num_fixed=0, seed=seed, outlier_frac=0.1, equirect=True)
    sel = sc["obs_pose"] == 1
    return dict(pose_cw=sc["pose_cw"][1], pos_w=sc["points_gt"][sc["obs_point"][sel]], uvr=sc["obs_uvr"][sel], inv_sigma_sq=sc["obs_inv_sigma_sq"][sel],
                huber=sc["obs_huber"][sel], intr=sc["intr"][1])


def _keep(n, kept):
    s = np.zeros(n, np.uint8)
    s[np.asarray(kept, int)] = 1
    return s


def _gross(src, n, good, seed):
    """the first n observations with all but `good` of them moved far off their projections"""
    rng = np.random.default_rng(seed)
    src = dict(src, uvr=src["uvr"][:n].copy())
    bad = rng.permutation(n)[good:]
    src["uvr"][bad, :2] += rng.uniform(150.0, 400.0, (len(bad), 2)).astype(np.float32) * rng.choice([-1.0, 1.0], (len(bad), 2)).astype(np.float32)
    return src


@functools.lru_cache(maxsize=None)
def classes():
    """{call: [problem, ...]}: the calls are "perspective", "stereo" and "equirect".  The lists are built once and shared: treat them as read-only."""
    # (seeds: the first of 20 + k, 100, 101, ... whose problem the oracle decides robustly, see oracle_is_decided)
    seeds = {63: 100, 65: 101, 513: 100}
    mono = [_pose_problem(seeds.get(n, 20 + k), n=max(n, 5) + 60) for k, n in enumerate(SIZES)]
    per = [_problem(f"size_{n}", f"{n} entries, all selected", mono[k], n) for k, n in enumerate(SIZES)]
    extra = _pose_problem(40, n=260)
    per.append(_problem("select_leaves_4", "40 entries of which select keeps 4: skipped", extra, 40, _keep(40, [3, 11, 12, 39])))
    per.append(_problem("select_leaves_5", "40 entries of which select keeps 5: optimised", _pose_problem(102, n=100, outlier_frac=0.0), 40, _keep(40, [0, 7, 8, 30, 39])))
    per.append(_problem("select_none", "20 entries, select all zeros: skipped", extra, 20, np.zeros(20, np.uint8)))
    per.append(_problem("select_every_second", "130 entries, select keeps every second: the compaction crosses waves", _pose_problem(42, n=200), 130,
                        _keep(130, np.arange(0, 130, 2))))
    per.append(_problem("early_break", "12 entries, 9 of them gross outliers: the oracle ends with n - num_bad < 5", _gross(_pose_problem(45, n=100, outlier_frac=0.0), 12, 3, 45), 12))
    per.append(_problem("inactive", "100 entries, active = 0: skipped", _pose_problem(44, n=160), 100, active=False))
    # mixed order: skipped problems between optimised ones, the largest neither first nor last
    order = ["size_65", "select_none", "size_513", "size_0", "select_every_second", "size_4", "size_1200", "inactive", "size_5", "early_break", "size_64",
             "select_leaves_4", "size_511", "size_63", "select_leaves_5", "size_512"]
    by = {p["name"]: p for p in per}
    assert sorted(order) == sorted(by)
    st_src = _pose_problem(50, n=400, stereo=True)
    stereo = [_problem("stereo_300", "300 stereo entries (u_right >= 0): three residual rows", st_src, 300),
              _problem("stereo_select", "70 stereo entries, select keeps every third", _pose_problem(51, n=130, stereo=True), 70, _keep(70, np.arange(0, 70, 3)))]
    eq = [_problem("equirect_300", "300 entries of an equirectangular camera (intr = 0 0 cols rows 0)", _equirect_source(60, 360), 300),
          _problem("equirect_select", "66 equirectangular entries, select drops the first and the last", _equirect_source(101, 130), 66, _keep(66, np.arange(1, 65)))]
    return dict(perspective=[by[k] for k in order], stereo=stereo, equirect=eq)


def selected(p):
    """the compacted arrays of a problem: what the callers hand to svgpu_pose_optimize one candidate at a time"""
    keep = np.ones(len(p["pos_w"]), bool) if p["select"] is None else p["select"] != 0
    return dict(pose_cw=p["pose_cw"], pos_w=p["pos_w"][keep], uvr=p["uvr"][keep], inv_sigma_sq=p["inv_sigma_sq"][keep], huber=p["huber"][keep], intr=p["intr"],
                keep=keep)


def oracle_is_decided(p, trials=6, sigma=1e-11):
    """A parity case must not sit on a decision of the optimisation that rounding settles: at a converged pose the gain rule of a further
    LM iteration, or a chi-square threshold, can be decided by the last bits of a sum, and two correct implementations then differ in
    iteration count or flags.  The oracle alone judges it: its iteration count, count of valid observations and flags have to stay the
    same when the starting pose moves by 1e-11 (far above the rounding of either implementation, far below anything that matters), for both
    readings of the stop flag.  A seed whose problem fails is replaced in classes()."""
    from oracle import oracle as O
    s = selected(p)
    if len(s["pos_w"]) < 5:
        return True
    rng = np.random.default_rng(1)
    for reset in (False, True):
        run = lambda pose: O.pose_optimize(pose, s["pos_w"], s["uvr"], s["inv_sigma_sq"], s["huber"], s["intr"], reset_flag_each_round=reset)
        nv, _, outl, st = run(s["pose_cw"])
        for _ in range(trials):
            nv2, _, outl2, st2 = run(s["pose_cw"] + rng.normal(0.0, sigma, 12))
            if nv2 != nv or st2[0] != st[0] or not np.array_equal(outl2, outl):
                return False
    return True


def is_skipped(p):
    return (not p["active"]) or int(selected(p)["keep"].sum()) < 5


def batch(problems, with_select=True, with_active=True):
    """flat arguments of optimize_batch_flat for a list of problems (of one camera)"""
    off = np.concatenate([[0], np.cumsum([len(p["pos_w"]) for p in problems])]).astype(np.int32)
    cat = lambda k, w, t: np.concatenate([np.asarray(p[k], t).reshape(-1, *w) for p in problems]) if problems else np.zeros((0, *w), t)
    sel = np.concatenate([np.ones(len(p["pos_w"]), np.uint8) if p["select"] is None else p["select"] for p in problems]) if problems else np.zeros(0, np.uint8)
    assert all(np.array_equal(p["intr"], problems[0]["intr"]) for p in problems)
    return dict(poses_cw=np.stack([p["pose_cw"] for p in problems]) if problems else np.zeros((0, 12)), obs_off=off, pos_w=cat("pos_w", (3,), np.float64),
                uvr=cat("uvr", (3,), np.float32), inv_sigma_sq=cat("inv_sigma_sq", (), np.float32), huber=cat("huber", (), np.float32),
                intr=problems[0]["intr"] if problems else np.array([500.0, 500.0, 320.0, 240.0, 0.0]), select=sel if with_select else None,
                active=np.array([p["active"] for p in problems], np.uint8) if with_active else None)
