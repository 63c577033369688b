"""Pose-optimiser problems on the chi-square gate and for ONE damped step (numpy + the CPU oracle only; tests/test_poseopt_problem_classes.py
holds every class to its claim).  The problems are shaped for the three entry points of stella_vslam_amd.optimize.pose_optimizer --
optimize_flat, optimize_device and optimize_batch_flat (batch_of lays a whole class list out as one batch call per camera).  The tracked-frame
chain and svgpu_reloc_refine_batch run the same kernel template; tests/test_gpu_track.py and tests/test_gpu_reloc_refine.py hold them
bit-equal to those entry points, so no problem here is shaped for them.

GATE problems are called with num_each_iter = 0: both the oracle and the kernel then only re-classify every edge at the INPUT pose.  The pose
is the identity rotation with a zero or dyadic translation, fx = fy = 512, the principal point and fxb are integers, the landmarks lie at
z in {1, 2, 4}: the projection is exact in doubles, and every observation is a float32 chosen so that the residual is the planted double
exactly.  chi2 = (r0 r0 + r1 r1 + r2 r2) * (double)w is then the same double on both sides, and the flags are planted, not measured:
  chi_on_threshold  residual 2 in one component, w = thr / 4 as a float: chi2 == (double)thr, an inlier because the test is strict; the
                    float neighbours of w on each side; the 2 in u, in v and (stereo) in the right-image component alone
  float_threshold   w = 1, one component whose square lies strictly between (double)5.99146f and the double 5.99146 (and the same for
                    7.81473): a gate against the double literal flips these; plants just outside the interval on each side do not flip
  threshold_choice  chi2 = 7 lies between the thresholds: an outlier as a monocular edge, an inlier as a stereo edge; u_right = -0.0f is
                    not "< 0": a stereo edge
  weight_widening   w of pyramid levels 1..7 (not dyadic): two residuals one unit in the last place of e apart, e e (double)w on either
                    side of the threshold
  sizes             n around the 512-thread stride, its tails and whole / partial waves; outliers at 0, n - 1 and the first and last index
                    of every stride pass, every other edge has chi2 == 0
  few               n = 4: nothing is classified; n = 5 with one outlier
STEP problems are called with one round of one iteration, with and without the Huber kernel: a small noisy scene, the initial pose a few
centimetres and tenths of a degree off, so that the first trial is accepted and the output is exp(dx) * T0 -- nothing corrects an error of
the sums, the 6 x 6 solve or the exponential.  restate_step is the step again in numpy longdouble, the high-precision reference of the
oracle's step; every problem also has its reversed-observation copy (the same sums in another order: the oracle's own noise).
"""
import functools

import numpy as np

from oracle import oracle as O

F32 = np.float32
THR_MONO, THR_STEREO = F32(5.99146), F32(7.81473)      # what the reference compares against, widened
THR_MONO_DOUBLE, THR_STEREO_DOUBLE = 5.99146, 7.81473  # what a gate written with double literals would compare against
K_IMG = np.array([512.0, 512.0, 320.0, 240.0, 32.0])   # fx fy cx cy fxb
K_ORIGIN = np.array([512.0, 512.0, 0.0, 0.0, 32.0])    # principal point 0: a projection takes every double, not only those near cx
IDENTITY = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
STRIDE = 512                                            # threads of k_pose_opt: edge i is thread i % 512's in pass i // 512
GATE_SCHEDULES = ((2, 2, 0), (1, 0, 0))                 # (num_trials_robust, num_trials, num_each_iter)
STEP_SCHEDULES = dict(huber=(1, 0, 1), plain=(0, 1, 1))
OBS_KEYS = ("pos_w", "uvr", "inv_sigma_sq", "huber")


def threshold(u_right) -> np.float32:
    return THR_MONO if u_right < 0 else THR_STEREO


def chi2_numpy(res, w):
    """chi2 in the oracle's operation order, in float64"""
    r = np.asarray(res, np.float64).reshape(-1, 3)
    return (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]) * np.asarray(w, np.float32).astype(np.float64)


def _project(intr, pc):
    x, y, z = (np.float64(c) for c in pc)
    u = intr[0] * x / z + intr[2]
    v = intr[1] * y / z + intr[3]
    return u, v, u - intr[4] / z


class _Gate:
    """A gate problem under construction: plant(pc, res, w, claim) adds the edge whose landmark lies at pc in the camera and whose
    residual is `res`; `claim` is the flag the class says it gets."""

    def __init__(self, name, cls, intr=K_IMG, t=(0.0, 0.0, 0.0)):
        self.name, self.cls, self.intr, self.t, self.rows = name, cls, np.array(intr, np.float64), np.array(t, np.float64), []

    def plant(self, pc, res, w, claim, stereo, right=None, **tags):
        pc, res = np.array(pc, np.float64), np.array(res, np.float64)
        u, v, ur = _project(self.intr, pc)
        uvr = np.array([u + res[0], v + res[1], (ur + res[2]) if stereo else -1.0], np.float32)
        if right is not None:
            uvr[2] = right
        assert stereo or res[2] == 0.0
        pos_w = pc - self.t
        assert np.array_equal(pos_w + self.t, pc)   # the translation is exact
        self.rows.append(dict(pos_w=pos_w, uvr=uvr, w=F32(w), res=res, claim=int(claim), **tags))

    def done(self):
        n = len(self.rows)
        col = lambda k, t, w: np.array([r[k] for r in self.rows], t).reshape(n, *w)
        pose = IDENTITY.copy()
        pose[[3, 7, 11]] = self.t
        uvr = col("uvr", np.float32, (3,))
        tags = [{k: v for k, v in r.items() if k in ("inside", "pair")} for r in self.rows]
        return dict(name=self.name, cls=self.cls, pose_cw=pose, intr=self.intr, pos_w=col("pos_w", np.float64, (3,)), uvr=uvr,
                    inv_sigma_sq=col("w", np.float32, ()), huber=np.sqrt(np.where(uvr[:, 2] < 0, THR_MONO, THR_STEREO)).astype(np.float32),
                    residual=col("res", np.float64, (3,)), claim=col("claim", np.uint8, ()), tags=tags)


def _dyadic_points(k):
    """camera-frame points at z in {1, 2, 4} with multiples of 1/8 as x, y; x >= -z / 2 keeps the right-image coordinate positive"""
    z = (1.0, 2.0, 4.0)[k % 3]
    return np.array([((k * 5) % 13 - 4) / 8.0 * z, ((k * 7) % 11 - 5) / 8.0, z])


def _chi_on_threshold():
    g = _Gate("chi_on_threshold", "chi_on_threshold", t=(0.5, -0.25, 0.0))
    k = 0
    for stereo in (False, True):
        thr = THR_STEREO if stereo else THR_MONO
        w = F32(thr / F32(4))
        assert float(w) * 4.0 == float(thr)
        for comp in range(3 if stereo else 2):
            res = np.zeros(3)
            res[comp] = 2.0 if k % 2 == 0 else -2.0
            for ww, claim in ((np.nextafter(w, F32(0)), 0), (w, 0), (np.nextafter(w, F32(np.inf)), 1)):
                g.plant(_dyadic_points(k), res, ww, claim, stereo)
                k += 1
    return g.done()


def _float_threshold():
    g = _Gate("float_threshold", "float_threshold")
    k = 0
    for thr32, thr64, stereo in ((THR_MONO, THR_MONO_DOUBLE, False), (THR_STEREO, THR_STEREO_DOUBLE, True)):
        lo, hi = sorted((float(thr32), thr64))
        targets = [(lo + f * (hi - lo), True) for f in (0.25, 0.5, 0.75)] + [(lo - 0.5 * (hi - lo), False), (hi + 0.5 * (hi - lo), False)]
        for target, inside in targets:
            for comp in ((0, 1) if not stereo else (1,)):   # (a stereo edge's u cannot move alone: the right-image residual would follow)
                z = (1.0, 2.0, 4.0)[k % 3]
                c = g.intr[2 + comp]
                proj = c - np.sqrt(target)                  # a double next to the principal point: the residual c - proj has its grain, ~6e-14
                pc = np.array([0.5 * z, 0.25 * z, z])
                pc[comp] = (proj - c) * z / 512.0
                res = np.zeros(3)
                res[comp] = c - proj
                u, v, ur = _project(g.intr, pc)
                assert (u, v)[comp] == proj
                chi = float(chi2_numpy(res, 1.0)[0])
                assert (lo < chi < hi) == inside
                g.plant(pc, res, 1.0, float(thr32) < chi, stereo, inside=inside)
                g.rows[-1]["uvr"][comp] = c                 # the observation is the principal point itself
                k += 1
    return g.done()


def _threshold_choice():
    g = _Gate("threshold_choice", "threshold_choice", t=(-0.125, 0.5, 0.0))
    for k in range(3):
        pc = _dyadic_points(k)
        for comp in (0, 1):
            res = np.zeros(3)
            res[comp] = 2.0
            g.plant(pc, res, 1.75, 1, False)   # chi2 = 7 against 5.99146
            g.plant(pc, res, 1.75, 0, True)    #          against 7.81473
    # u_right = -0.0f: "-0.0 < 0" is false, the edge is a stereo edge.  u - fxb / z == 0 here, so its right-image residual is -0.0 - 0.0
    pc = np.array([(32.0 - 320.0) / 512.0, 0.125, 1.0])
    assert _project(g.intr, pc)[2] == 0.0
    g.plant(pc, [0.0, 2.0, -0.0], 1.75, 0, True, right=F32(-0.0))
    assert np.signbit(g.rows[-1]["uvr"][2])
    return g.done()


def _weight_widening():
    g = _Gate("weight_widening", "weight_widening", intr=K_ORIGIN)
    inv_level_sigma_sq = O.scale_tables(1.2, 8)[3]
    for level in range(1, 8):
        w, stereo = inv_level_sigma_sq[level], level % 2 == 0
        thr, comp = float(THR_STEREO if stereo else THR_MONO), (1 if stereo else (level // 2) % 2)
        chi = lambda e: float(e * e * np.float64(w))
        e = np.sqrt(np.float64(thr) / np.float64(w))
        while chi(e) > thr:
            e = np.nextafter(e, 0.0)
        while chi(np.nextafter(e, np.inf)) <= thr:
            e = np.nextafter(e, np.inf)
        for ee, claim in ((e, 0), (np.nextafter(e, np.inf), 1)):   # one unit in the last place of e apart
            obs = 2.0 ** np.ceil(np.log2(ee))                       # e in [obs / 2, obs): obs - e is exact, and so is obs - (obs - e)
            z = (1.0, 2.0, 4.0)[level % 3]
            pc = np.array([0.5 * z, 0.25 * z, z])
            pc[comp] = (obs - ee) * z / 512.0
            res = np.zeros(3)
            res[comp] = ee
            assert _project(g.intr, pc)[comp] == obs - ee and obs - (obs - ee) == ee
            g.plant(pc, res, w, claim, stereo, pair=level)
    return g.done()


def stride_outliers(n):
    """index 0, n - 1, and the first and last index of every pass of the 512-thread stride"""
    idx = {0, n - 1}
    for first in range(0, n, STRIDE):
        idx |= {first, min(first + STRIDE, n) - 1}
    return sorted(idx)


SIZES = (5, 63, 64, 65, 511, 512, 513, 1024, 1025, 1537)


def _size(n, outliers, name, cls="sizes"):
    g = _Gate(name, cls, t=(0.5, -0.25, 0.0) if n % 2 else (0.0, 0.0, 0.0))
    out = set(outliers)
    for i in range(n):
        stereo = i % 3 != 1
        res = np.zeros(3)
        if i in out:
            res[i % (3 if stereo else 2)] = 8.0 if i % 2 else -8.0   # chi2 = 64
        g.plant(_dyadic_points(i), res, 1.0, i in out and n >= 5, stereo)   # (below 5 edges nothing is classified)
    return g.done()


@functools.lru_cache(None)
def gate_problems():
    """every gate problem, built once; read-only"""
    ps = [_chi_on_threshold(), _float_threshold(), _threshold_choice(), _weight_widening()]
    ps += [_size(n, stride_outliers(n), f"size_{n}") for n in SIZES]
    ps += [_size(4, (0, 1, 2), "few_4", "few"), _size(5, (2,), "few_5", "few")]
    return ps


def gate_by_name(name):
    return next(p for p in gate_problems() if p["name"] == name)


GATE_NAMES = ["chi_on_threshold", "float_threshold", "threshold_choice", "weight_widening"] + [f"size_{n}" for n in SIZES] + ["few_4", "few_5"]


def planted_flags(p):
    """the flags a problem is planted to get: numpy float64 in the oracle's operation order; nothing below 5 edges"""
    if len(p["pos_w"]) < 5:
        return np.zeros(len(p["pos_w"]), np.uint8)
    thr = np.where(p["uvr"][:, 2] < 0, THR_MONO, THR_STEREO).astype(np.float64)
    return (thr < chi2_numpy(p["residual"], p["inv_sigma_sq"])).astype(np.uint8)


def oracle_edge(p, i, pose=None):
    """(residual[3], rows) of edge i at `pose` (default: the problem's own), from the oracle's own edge code"""
    lib = O.lib()
    T = np.asarray(p["pose_cw"] if pose is None else pose, np.float64).reshape(3, 4)
    q, t = np.zeros(4), np.zeros(3)
    lib.orc_dbg_se3_from_Rt(O._p(np.ascontiguousarray(T[:, :3])), O._p(np.ascontiguousarray(T[:, 3])), O._p(q), O._p(t))
    err, A, B = np.zeros(3), np.zeros(9), np.zeros(18)
    D = lib.orc_dbg_reproj_edge(O._p(q), O._p(t), O._p(np.ascontiguousarray(p["pos_w"][i])), O._p(p["intr"]), O._p(np.ascontiguousarray(p["uvr"][i])),
                                O._p(err), O._p(A), O._p(B))
    return err, D   # (an int: ctypes' default return type)


def oracle_chi2(p, pose):
    """chi2 of every edge at `pose` from the oracle's own residuals (po_chi's operation order)"""
    return chi2_numpy(np.stack([oracle_edge(p, i, pose)[0] for i in range(len(p["pos_w"]))]), p["inv_sigma_sq"])


def oracle_run(p, schedule, reverse=False):
    """(num_valid, pose, flags, lm_iterations) of the oracle; `reverse`: on the reversed-observation copy, the flags turned back"""
    s = slice(None, None, -1) if reverse else slice(None)
    nv, pose, outl, st = O.pose_optimize(p["pose_cw"], p["pos_w"][s], p["uvr"][s], p["inv_sigma_sq"][s], p["huber"][s], p["intr"], num_trials_robust=schedule[0],
                                         num_trials=schedule[1], num_each_iter=schedule[2])
    return int(nv), pose, np.ascontiguousarray(outl[s]), int(st[0])


# ------------------------------------------------------------------------------------------- the batch form

def _junk(intr):
    """an entry that would be an outlier if it were selected"""
    u, v, ur = _project(intr, (0.25, 0.125, 1.0))
    return dict(pos_w=np.array([0.25, 0.125, 1.0]), uvr=np.array([u + 48.0, v - 48.0, ur], np.float32), inv_sigma_sq=F32(1.0), huber=F32(2.0))


def with_gaps(p, seed, keep_only=None):
    """The problem as a slice of a batch: unselected entries (gross outliers, were they selected) stand before, between and behind the
    planted ones, so the device's compaction moves every planted entry.  Returns the entry arrays, `select` and the pose; the entries
    where select != 0 are the problem's, in order.  keep_only: select only that many of the problem's edges (the rest become unselected)."""
    rng = np.random.default_rng(seed)
    n = len(p["pos_w"])
    gaps = rng.integers(0, 3, n + 1) * (rng.random(n + 1) < 0.4)
    gaps[0] = max(gaps[0], 1)
    j = _junk(p["intr"])
    cols = {k: [] for k in OBS_KEYS}
    select = []
    for i in range(n + 1):
        for _ in range(int(gaps[i])):
            for k in OBS_KEYS:
                cols[k].append(j[k])
            select.append(0)
        if i < n:
            for k in OBS_KEYS:
                cols[k].append(p[k][i])
            select.append(1 if keep_only is None or i < keep_only else 0)
    out = dict(name=p["name"], pose_cw=p["pose_cw"], intr=p["intr"], select=np.array(select, np.uint8), active=True)
    out["pos_w"] = np.array(cols["pos_w"], np.float64).reshape(-1, 3)
    out["uvr"] = np.array(cols["uvr"], np.float32).reshape(-1, 3)
    out["inv_sigma_sq"], out["huber"] = np.array(cols["inv_sigma_sq"], np.float32), np.array(cols["huber"], np.float32)
    return out


def batch_of(problems, seed):
    """One optimize_batch_flat call over `problems` (of one camera) in shuffled order, with an empty problem, an inactive one and one with
    fewer than 5 selected entries among them.  Returns (arguments, members): members[k] = (name or None, slice of the entries, select, active,
    input pose)."""
    assert all(np.array_equal(p["intr"], problems[0]["intr"]) for p in problems)
    src = problems[0]
    donor = max(problems, key=lambda p: len(p["pos_w"]))
    members = [with_gaps(p, seed + k) for k, p in enumerate(problems)]
    empty = dict(name=None, pose_cw=src["pose_cw"], select=np.zeros(0, np.uint8), active=True, pos_w=np.zeros((0, 3)), uvr=np.zeros((0, 3), np.float32),
                 inv_sigma_sq=np.zeros(0, np.float32), huber=np.zeros(0, np.float32))
    inactive = dict(with_gaps(donor, seed + 100), name=None, active=False)
    under5 = dict(with_gaps(donor, seed + 101, keep_only=4), name=None)
    members += [empty, inactive, under5]
    order = np.random.default_rng(seed).permutation(len(members))
    members = [members[k] for k in order]
    off = np.concatenate([[0], np.cumsum([len(m["select"]) for m in members])]).astype(np.int32)
    args = dict(poses_cw=np.stack([m["pose_cw"] for m in members]), obs_off=off, intr=src["intr"], select=np.concatenate([m["select"] for m in members]),
                active=np.array([m["active"] for m in members], np.uint8))
    for k in OBS_KEYS:
        args[k] = np.concatenate([m[k] for m in members])
    return args, [(m["name"], slice(int(off[k]), int(off[k + 1])), m["select"], m["active"], m["pose_cw"]) for k, m in enumerate(members)]


def cameras(problems):
    """the problems grouped by their intrinsics (a batch call has one camera)"""
    groups = {}
    for p in problems:
        groups.setdefault(p["intr"].tobytes(), []).append(p)
    return list(groups.values())


# ------------------------------------------------------------------------------------------- one damped step

def _rodrigues(w):
    th = np.linalg.norm(w)
    Om = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / th ** 2 * Om @ Om


def _unit(rng, k=3):
    v = rng.normal(size=k)
    return v / np.linalg.norm(v)


def project_numpy(T, intr, pos_w, dtype=np.float64):
    """(u, v, u_right, pc) of the landmarks at pose T (3 x 4) in `dtype`"""
    T, K = np.asarray(T, dtype).reshape(3, 4), np.asarray(intr, dtype)
    pc = np.asarray(pos_w, dtype) @ T[:, :3].T + T[:, 3]
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    if K[0] == 0 and K[1] == 0:
        pi = dtype(np.pi)   # the function under test is written with the double M_PI
        theta, phi = np.arctan2(x, z), -np.arcsin(y / np.sqrt(x * x + y * y + z * z))
        u, v = K[2] * (dtype(0.5) + theta / (2 * pi)), K[3] * (dtype(0.5) - phi / pi)
    else:
        u, v = K[0] * x / z + K[2], K[1] * y / z + K[3]
    return u, v, u - K[4] / z, pc


def residuals_numpy(T, p, dtype=np.float64):
    u, v, ur, pc = project_numpy(T, p["intr"], p["pos_w"], dtype)
    o = p["uvr"].astype(dtype)
    eq = p["intr"][0] == 0 and p["intr"][1] == 0
    stereo = ~(p["uvr"][:, 2] < 0) & (not eq)
    r = np.stack([o[:, 0] - u, o[:, 1] - v, np.where(stereo, o[:, 2] - ur, dtype(0))], 1)
    return r, pc, stereo


def _step_problem(name, cls, n, seed, camera="mono", huber_off_third=False, huber_planted=False, rot_off=4e-3, trans_off=0.03, noise=1.0, depth=(3.0, 12.0),
                  min_move=1e-3):
    """min_move: the least |pose_out - pose_in| (largest entry) the class test asks of the step; a tenth of the initial offset or less"""
    rng = np.random.default_rng(seed)
    R_gt, t_gt = _rodrigues(_unit(rng) * 0.4), rng.uniform(-1.0, 1.0, 3)
    eq = camera == "equirect"
    intr = np.array([0.0, 0.0, 1920.0, 960.0, 0.0]) if eq else np.array([520.3, 515.7, 318.2, 242.9, 41.6 if camera in ("stereo", "mixed") else 0.0])
    z = rng.uniform(*depth, n)
    if eq:
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[:, 1] *= 0.6   # away from the poles
        pc = d / np.linalg.norm(d, axis=1, keepdims=True) * z[:, None]
    else:
        pc = np.stack([(rng.uniform(20, 620, n) - intr[2]) * z / intr[0], (rng.uniform(20, 460, n) - intr[3]) * z / intr[1], z], 1)
    pos_w = (pc - t_gt) @ R_gt   # R^T (pc - t)
    pose_gt = np.concatenate([R_gt, t_gt[:, None]], 1).reshape(12)
    R_off = _rodrigues(_unit(rng) * rot_off)
    pose0 = np.concatenate([R_off @ R_gt, (R_off @ t_gt + _unit(rng) * trans_off)[:, None]], 1).reshape(12)
    sf, _, _, inv_sigma_sq = O.scale_tables(1.2, 8)
    level = rng.integers(0, 8, n)
    stereo = np.zeros(n, bool) if camera in ("mono", "equirect") else (np.ones(n, bool) if camera == "stereo" else np.arange(n) % 2 == 0)
    planted = np.zeros(n, bool)
    if huber_planted:   # the planted third comes in pairs on one landmark, level and edge kind (see below)
        planted = np.arange(n) % 3 == 1
        ka, kb = np.flatnonzero(planted)[0::2], np.flatnonzero(planted)[1::2]
        assert len(ka) == len(kb)
        pos_w[kb], level[kb], stereo[kb] = pos_w[ka], level[ka], stereo[ka]
    w = inv_sigma_sq[level].astype(np.float32)
    u, v, ur, _ = project_numpy(pose_gt, intr, pos_w)
    e = rng.normal(size=(n, 3)) * (noise * sf[level].astype(np.float64))[:, None]
    uvr = np.stack([u + e[:, 0], v + e[:, 1], np.where(stereo, ur + e[:, 2], -1.0)], 1)
    huber = np.sqrt(np.where(stereo, THR_STEREO, THR_MONO)).astype(np.float32)
    if huber_planted:
        # A third of the edges at 2 .. 4 delta^2 AT THE INITIAL POSE: the branch e > delta^2 of the kernel, beside the other two thirds in
        # e <= delta^2.  The two edges of a pair lie opposite each other around the landmark's projection at the initial pose: their terms
        # of b cancel (the step still points at the true pose), their terms of H do not.
        u0, v0, ur0, _ = project_numpy(pose0, intr, pos_w)
        mag = np.sqrt(rng.uniform(2.0, 4.0, len(ka)) * huber[ka].astype(np.float64) ** 2 / w[ka].astype(np.float64))
        dirs = np.stack([_unit(rng, 3) for _ in ka])
        dirs[~stereo[ka], 2] = 0.0
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        for k, sign in ((ka, 1.0), (kb, -1.0)):
            uvr[k, 0], uvr[k, 1] = u0[k] + sign * mag * dirs[:, 0], v0[k] + sign * mag * dirs[:, 1]
            uvr[k, 2] = np.where(stereo[k], ur0[k] + sign * mag * dirs[:, 2], -1.0)
    if huber_off_third:
        huber[0::6], huber[3::6] = 0.0, -1.0
    assert (uvr[stereo, 2] >= 0).all()
    return dict(name=name, cls=cls, pose_cw=pose0, pose_gt=pose_gt, intr=intr, pos_w=np.ascontiguousarray(pos_w), uvr=np.ascontiguousarray(uvr, np.float32),
                inv_sigma_sq=w, huber=huber, planted=planted, min_move=min_move)


STEP_SIZES = (5, 6, 64, 65, 512, 513, 1025)
_STEP = [
    ("mono", lambda: _step_problem("mono", "camera", 150, 201)),
    ("stereo", lambda: _step_problem("stereo", "camera", 150, 202, camera="stereo")),
    ("equirect", lambda: _step_problem("equirect", "camera", 150, 203, camera="equirect")),
    ("mixed", lambda: _step_problem("mixed", "camera", 151, 204, camera="mixed")),
    ("no_kernel_third", lambda: _step_problem("no_kernel_third", "huber", 150, 205, camera="mixed", huber_off_third=True)),
    ("huber_planted", lambda: _step_problem("huber_planted", "huber", 150, 206, camera="mixed", huber_planted=True, rot_off=1e-3, trans_off=5e-3, noise=0.3,
                                            depth=(5.0, 12.0), min_move=1e-4)),
    # (huber_planted starts 5 mm / 0.06 degrees off, a sixth of the others, so that every unplanted edge lies below delta^2 at the initial
    #  pose; the planted pairs add stiffness and no gradient, which shortens the step further: its least movement is scaled alike)
] + [(f"size_{n}", (lambda n=n, k=k: _step_problem(f"size_{n}", "sizes", n, 210 + k, noise=1.0 if n > 6 else 0.1))) for k, n in enumerate(STEP_SIZES)]
# (five or six points with a pixel of noise do not fix a pose to centimetres: the step would not approach the true pose; a tenth of a pixel there)
STEP_NAMES = [k for k, _ in _STEP]


@functools.lru_cache(None)
def step_problem(name):
    """built once per process; read-only"""
    return dict(_STEP)[name]()


def reversed_copy(p):
    out = dict(p)
    for k in OBS_KEYS:
        out[k] = np.ascontiguousarray(p[k][::-1])
    return out


@functools.lru_cache(None)
def step_reference(name, mode):
    """(the oracle's (num_valid, pose, flags, iterations), its reorder spread on the pose entries): spread = max|delta| between the problem
    and its reversed-observation copy"""
    p = step_problem(name)
    ref, rev = oracle_run(p, STEP_SCHEDULES[mode]), oracle_run(p, STEP_SCHEDULES[mode], reverse=True)
    return ref, float(np.abs(ref[1] - rev[1]).max())


def gate_chi2_after(p, pose):
    """(chi2 of every edge at `pose`, its threshold), float64"""
    r, _, _ = residuals_numpy(pose, p)
    return chi2_numpy(r, p["inv_sigma_sq"]), np.where(p["uvr"][:, 2] < 0, THR_MONO, THR_STEREO).astype(np.float64)


def _solve_spd(A, b):
    """LL^T solve in the dtype of A"""
    n = len(b)
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] * L[j, :j]).sum())
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


def restate_step(p, robust, dtype=np.longdouble):
    """One damped step restated plainly in `dtype`: residuals, the rows d e / d [omega, upsilon] of the three edge kinds, Huber,
    lambda = 1e-5 max diag H, the damped 6 x 6 solve, exp(dx) * T0.  Returns (pose 3 x 4 flat as float64, dx, robust chi2 before, after)."""
    D = dtype
    r, pc, stereo = residuals_numpy(p["pose_cw"], p, D)
    K = p["intr"].astype(D)
    n = len(r)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    J = np.zeros((n, 3, 6), D)
    if K[0] == 0 and K[1] == 0:
        pi = D(np.pi)
        L, rxz = np.sqrt(x * x + y * y + z * z), x * x + z * z
        zero, one = np.zeros(n, D), np.ones(n, D)
        dX, dY, dZ = [zero, z, -y, one, zero, zero], [-z, zero, x, zero, one, zero], [y, -x, zero, zero, zero, one]
        for k in range(6):
            dL = (x * dX[k] + y * dY[k] + z * dZ[k]) / L
            J[:, 0, k] = -(K[2] / (2 * pi)) / rxz * (z * dX[k] - x * dZ[k])
            J[:, 1, k] = -(K[3] / pi) / (L * np.sqrt(rxz)) * (L * dY[k] - y * dL)
    else:
        fx, fy, fxb, zz = K[0], K[1], K[4], z * z
        J[:, 0] = np.stack([x * y / zz * fx, -(1 + x * x / zz) * fx, y / z * fx, -1 / z * fx, 0 * z, x / zz * fx], 1)
        J[:, 1] = np.stack([(1 + y * y / zz) * fy, -x * y / zz * fy, -x / z * fy, 0 * z, -1 / z * fy, y / zz * fy], 1)
        J[:, 2] = np.stack([J[:, 0, 0] - fxb * y / zz, J[:, 0, 1] + fxb * x / zz, J[:, 0, 2], J[:, 0, 3], 0 * z, J[:, 0, 5] - fxb / zz], 1)
        J[~stereo, 2] = 0
    w0, delta = p["inv_sigma_sq"].astype(D), p["huber"].astype(D)

    def rho(rr):
        chi = (rr * rr).sum(1) * w0
        kern = (delta > 0) & bool(robust)
        over = kern & (chi > delta * delta)
        s = np.sqrt(np.where(over, chi, D(1)))
        return np.where(over, 2 * s * delta - delta * delta, chi), np.where(over, delta / s, D(1))

    rho0, rho1 = rho(r)
    w = w0 * rho1
    H = np.einsum("nda,n,ndc->ac", J, w, J)
    b = -np.einsum("nda,n,nd->a", J, w, r)
    lam = D(1e-5) * np.abs(np.diag(H)).max()
    dx = _solve_spd(H + lam * np.eye(6, dtype=D), b)
    om, up = dx[:3], dx[3:]
    th = np.sqrt((om * om).sum())
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]], D)
    if th < 1e-5:
        a, bb, d = D(1), D(0.5), D(1) / 6
    else:
        a, bb, d = np.sin(th) / th, (1 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th * th * th)
    I = np.eye(3, dtype=D)
    R, V = I + a * Om + bb * (Om @ Om), I + bb * Om + d * (Om @ Om)
    T0 = p["pose_cw"].astype(D).reshape(3, 4)
    T1 = np.concatenate([R @ T0[:, :3], (R @ T0[:, 3] + V @ up)[:, None]], 1)
    r1, _, _ = residuals_numpy(T1, p, D)
    return T1.astype(np.float64).reshape(12), dx.astype(np.float64), float(rho0.sum()), float(rho(r1)[0].sum())
