"""Planted problems for the projection family (frame_device.h: project_to_image, reproject_one, reproject_window; k_grid_walk; the stereo
and chi-square gates of the candidate matcher), one class per gate.  numpy + oracle.oracle only: shared by the CPU class test and the
device parity test, which hands in its own `backend` (a dict of callables with the oracle wrappers' signatures).

Every boundary sits where the deciding quantity is exact in IEEE arithmetic, so device and oracle have to agree bit for bit:
  * cameras without distortion, fx = fy = 512, integer cx / cy, 1024 x 768 on the 64 x 48 grid (a cell is 16 px, inv_w = 1/16);
    compute_image_bounds then yields exactly 0, cols, 0, rows (asserted in `oracle_cam`);
  * identity rotation, zero translation; landmarks at Z in {1, 2, 4} with dyadic X, Y, so fx * X * z_inv + cx has no rounding away from
    the planted step; distance and normal classes use on-axis points (0, 0, Z), where sqrt((0 + 0) + Z * Z) == Z;
  * a gate is observed through a matcher by a PRIVATE keypoint per landmark: the landmark's own descriptor (Hamming distance 0) at the
    landmark's reprojection.  match[i] is then that keypoint iff landmark i passed its gates.
    Wherever the geometry leaves the image point free the keypoints lie in cells of their own, more than two margins apart.  Three
    classes cannot: distance_double, half_dot and sim3_center need |v| == Z exactly, which only an on-axis point gives under the identity
    pose, so all their landmarks reproject to (cx, cy) and all their keypoints lie there.  In those classes every landmark sees every
    keypoint inside its window, and the descriptors alone tell them apart; the window and margin gates have classes of their own.
Descriptors are rows of the 256 x 256 Sylvester-Hadamard matrix: any two differ in EXACTLY 128 bits.  (More than 128 for dozens of
256-bit codes would need a Plotkin-optimal code; 128 is beyond every threshold of the family -- 50 and 100 -- which is what isolates.)
Each triple (below / on / above a boundary) carries its expected outcome from the reference's text as cited in frame_device.h,
frame_kernels.h and oracle/match2_oracle.c; tests/test_reproj_problem_classes.py holds the oracle to it.

Boundaries left out because they cannot be made exact: an on-axis point at the smallest positive Z (0 * inf: a NaN whose sign and
payload IEEE leaves open -- the tiny-Z plants are off axis instead, where the image point is +inf); everything that needs libm on
the boundary (equirectangular positions, undistortion, acos) as the issue lists."""
import numpy as np

from oracle import oracle as O

W, H, FX, CX, CY = 1024, 768, 512.0, 512.0, 384.0
LEVELS = 8
SF, _, _, INV_SIGMA_SQ = O.scale_tables(1.2, LEVELS)
LSF = float(np.float32(np.log(np.float32(1.2))))     # std::log(float) of the reference's orb_params
f32, f64 = np.float32, np.float64
MATCHERS = ("current_last", "frame_keyframe", "sim3", "mutually", "fuse")
ENTRY_POINTS = ("reproject_landmarks",) + MATCHERS
PINHOLE = ("perspective", "fisheye", "radial_division")
_MODEL = dict(perspective=O.CAM_PERSPECTIVE, fisheye=O.CAM_FISHEYE, radial_division=O.CAM_RADIAL_DIVISION, equirectangular=O.CAM_EQUIRECTANGULAR)


def hadamard_desc(i):
    """row i + 1 of the Sylvester-Hadamard matrix of order 256 as 32 bytes"""
    j = np.arange(256)
    bits = np.array([bin((i + 1) & int(k)).count("1") & 1 for k in j], np.uint8)
    return np.packbits(bits)


def cam_spec(model, fxb=0.0, cols=W, rows=H, cx=CX, cy=CY):
    return dict(model=model, cols=cols, rows=rows, fx=FX, fy=FX, cx=cx, cy=cy, fxb=float(fxb))


def oracle_cam(spec):
    if spec["model"] == "equirectangular":
        return O.make_camera(O.CAM_EQUIRECTANGULAR, spec["cols"], spec["rows"])
    c = O.make_camera(_MODEL[spec["model"]], spec["cols"], spec["rows"], spec["fx"], spec["fy"], spec["cx"], spec["cy"], (0.0,) * 5, spec["fxb"])
    assert (c.min_x, c.max_x, c.min_y, c.max_y) == (0.0, float(spec["cols"]), 0.0, float(spec["rows"]))   # the bounds classes plant on these
    return c


def project(X, Y, Z, fxb=0.0, cx=CX, cy=CY):
    """perspective.cc:130-148 in the reference's operation order (every step an IEEE double operation)"""
    with np.errstate(all="ignore"):   # (the smallest positive Z: 1 / Z overflows to inf, as in the reference)
        z_inv = f64(1.0) / f64(Z)
        rx, ry = f64(FX) * f64(X) * z_inv + f64(cx), f64(FX) * f64(Y) * z_inv + f64(cy)
        return rx, ry, f32(rx - f64(fxb) * z_inv)


def predict_level(maxv, dist):
    """landmark::predict_scale_level (landmark.cc:336-353); callers keep away from ties (`level_q`) unless they plant an exact one"""
    lvl = int(np.ceil(f32(np.log(f64(f32(maxv) / f32(dist)))) / f32(LSF)))
    return 0 if lvl < 0 else min(lvl, LEVELS - 1)


def level_q(maxv, dist):
    return float(np.log(f64(f32(maxv)) / f64(f32(dist))) / LSF)


def coord_for(b, side, Z=1.0, c=CX):
    """the camera coordinate whose image coordinate FX * X / Z + c is the nearest reachable value below (-1), on (0) or above (+1) b"""
    X = (f64(b) - c) * f64(Z) / FX
    img = lambda x: f64(FX) * x * (f64(1.0) / f64(Z)) + f64(c)
    assert img(X) == b
    for _ in range(4):
        if side == 0 or (side < 0 and img(X) < b) or (side > 0 and img(X) > b):
            return float(X)
        X = np.nextafter(X, -np.inf if side < 0 else np.inf)
    raise AssertionError("no reachable image coordinate next to the boundary")


class Problem:
    """One call of one entry point: landmarks, keypoints and the expected match list."""

    def __init__(self, cls, ep, name, cam, margin=10.0, **opt):
        self.cls, self.ep, self.name, self.cam, self.margin, self.opt = cls, ep, name, cam, float(margin), opt
        self.lm, self.kp, self.expect, self.vis = [], [], [], []   # vis: the landmark passes its gates (what reproject_landmarks reports)
        self.lm2, self.expect2 = None, None   # match_keyframes_mutually: the landmarks of keyframe 2 (default: the same as keyframe 1's)
        self.exact_level = set()              # landmarks planted ON a level tie that is exact (scale_level)

    # ---- building
    def keypoint(self, x, y, octave, desc_id, xright=-1.0, occupied=0):
        self.kp.append(dict(xy=(f32(x), f32(y)), octave=int(octave), desc=hadamard_desc(desc_id), xright=f32(xright), occupied=occupied))
        return len(self.kp) - 1

    def landmark(self, pos, maxv=None, minv=None, normal=None, level=None, expect=True, kp="own", kp_octave=None, kp_xy=None, kp_xright=-1.0,
                 valid=1, has_obs=1, occupied=0, desc_id=None, ratio=1.1, lms=None, expects=None):
        """A landmark and (kp == "own") its private keypoint.  Without maxv the range is chosen around the distance so that the predicted
        level is 1 (ratio 1.1), clear of every other gate.  `expect`: the landmark passes, so match == its keypoint."""
        lms = self.lm if lms is None else lms
        expects = self.expect if expects is None else expects
        pos = np.asarray(pos, f64)
        dist = f64(np.sqrt((pos[0] * pos[0] + pos[1] * pos[1]) + pos[2] * pos[2]))
        if maxv is None:
            maxv = f32(dist * ratio)
        if minv is None:
            minv = f32(maxv) / f32(4.0)
        if normal is None:
            normal = pos / dist
        if level is None:
            level = predict_level(maxv, dist) if dist > 0 and np.isfinite(dist) and pos[2] > 0 else 0
        i = len(lms)
        desc_id = i + (100 if lms is not self.lm else 0) if desc_id is None else desc_id
        lms.append(dict(pos=pos, maxv=f32(maxv), minv=f32(minv), normal=np.asarray(normal, f64), level=int(level), valid=valid, has_obs=has_obs,
                        desc=hadamard_desc(desc_id), dist=dist))
        k = -1
        if kp == "own":
            rx, ry, _ = project(*pos, cx=self.cam["cx"], cy=self.cam["cy"]) if pos[2] > 0 else (f64(-100.0), f64(-100.0), 0)
            x, y = (rx, ry) if kp_xy is None else kp_xy
            if not (np.isfinite(x) and np.isfinite(y)):
                x, y = -100.0, -100.0
            k = self.keypoint(x, y, level if kp_octave is None else kp_octave, desc_id, kp_xright, occupied)
        elif kp is not None:
            k = int(kp)
        expects.append(k if expect else -1)
        if lms is self.lm:
            self.vis.append(bool(expect))
        return i

    def second_side(self):
        self.lm2, self.expect2 = [], []
        return dict(lms=self.lm2, expects=self.expect2)

    # ---- running
    def _lm_arrays(self, lms):
        n = len(lms)
        g = lambda k, t, w=(): np.array([l[k] for l in lms], t).reshape((n,) + w)
        return dict(pos_w=g("pos", f64, (3,)), valid=g("valid", np.uint8), min_valid_dist=g("minv", f32), max_valid_dist=g("maxv", f32),
                    mean_normal=g("normal", f64, (3,)), lm_desc=g("desc", np.uint8, (32,)), level=g("level", np.int32), has_obs=g("has_obs", np.uint8))

    def _kp_arrays(self, kps):
        n = len(kps)
        g = lambda k, t, w=(): np.array([p[k] for p in kps], t).reshape((n,) + w)
        return dict(tdesc=g("desc", np.uint8, (32,)), t_xy=g("xy", f32, (2,)), t_octave=g("octave", np.int32), t_xright=g("xright", f32),
                    occupied=g("occupied", np.uint8))

    def run(self, backend):
        """-> tuple of result arrays / counts as the entry point returns them"""
        cam = backend["cam"](self.cam)
        L, K = self._lm_arrays(self.lm), self._kp_arrays(self.kp)
        R, t = np.eye(3), np.zeros(3)
        tab = dict(scale_factors=SF, log_scale_factor=LSF, margin=self.margin)
        kps = dict(tdesc=K["tdesc"], t_xy=K["t_xy"], t_octave=K["t_octave"])
        rng = dict(min_valid_dist=L["min_valid_dist"], max_valid_dist=L["max_valid_dist"])
        ep = self.ep
        if ep == "reproject_landmarks":
            return backend[ep](cam, R, t, L["pos_w"], L["mean_normal"], L["min_valid_dist"], L["max_valid_dist"], 0.5, LEVELS, LSF, L["valid"])
        if ep == "current_last":
            stereo = self.cam["fxb"] != 0
            return backend[ep](self.opt.get("check_orientation", False), cam, rot_cw=R, trans_cw=t, rot_lw=R, trans_lw=np.asarray(self.opt.get("trans_lw", t), f64),
                               pos_w=L["pos_w"], valid=L["valid"], lm_desc=L["lm_desc"], octave_last=L["level"], angle_last=np.zeros(len(self.lm), f32),
                               scale_factors=SF, margin=self.margin, t_angle=np.zeros(len(self.kp), f32), occupied=K["occupied"],
                               t_xright=K["t_xright"] if stereo else None, lm_has_observation=L["has_obs"], is_monocular=not stereo,
                               true_baseline=float(self.opt.get("true_baseline", self.cam["fxb"] / FX)), **kps)
        if ep == "frame_keyframe":
            return backend[ep](False, cam, rot_cw=R, trans_cw=t, pos_w=L["pos_w"], valid=L["valid"], lm_desc=L["lm_desc"], angle_kf=np.zeros(len(self.lm), f32),
                               hamm_dist_thr=100, t_angle=np.zeros(len(self.kp), f32), occupied=K["occupied"], **rng, **tab, **kps)
        if ep == "sim3":
            sim3 = np.eye(4)
            sim3[:3, :3] *= 2.0   # a power of two: the reference's division by the scale (projection.cc:326-330) is exact
            return backend[ep](cam, sim3_cw=sim3, pos_w=L["pos_w"], valid=L["valid"], mean_normal=L["mean_normal"], lm_desc=L["lm_desc"],
                               occupied=K["occupied"], **rng, **tab, **kps)
        if ep == "fuse":
            stereo = self.cam["fxb"] != 0
            return backend[ep](cam, rot_cw=R, trans_cw=t, pos_w=L["pos_w"], valid=L["valid"], mean_normal=L["mean_normal"], lm_desc=L["lm_desc"],
                               inv_level_sigma_sq=INV_SIGMA_SQ, t_xright=K["t_xright"] if stereo else None,
                               do_reprojection_matching=bool(self.opt.get("reproj", False)), **rng, **tab, **kps)
        assert ep == "mutually"
        kf1, kf2, cam1 = self.sides()
        return backend[ep](backend["cam"](cam1), cam, rot_1w=R, trans_1w=t, rot_2w=R, trans_2w=t, s_12=float(self.opt.get("s_12", 1.0)), rot_12=R,
                           trans_12=np.asarray(self.opt.get("trans_12", t), f64), kf1=kf1, kf2=kf2, **tab)

    def sides(self):
        """keyframe 1 carries self.lm and the private keypoints of keyframe 2's landmarks; keyframe 2 the reverse.  A keyframe has one
        landmark slot per keypoint, so the shorter of (landmarks, keypoints) is padded: invalid landmarks / keypoints outside the grid."""
        lm2 = self.lm if self.lm2 is None else self.lm2
        kp1 = self.opt.get("kp1", self.kp)      # keypoints of keyframe 1 = private keypoints of lm2
        kp2 = self.kp

        def side(lms, kps):
            lms, kps = list(lms), list(kps)
            while len(lms) < len(kps):
                lms.append(dict(pos=np.zeros(3), maxv=f32(1), minv=f32(1), normal=np.zeros(3), level=0, valid=0, has_obs=1, desc=hadamard_desc(254), dist=0.0))
            while len(kps) < len(lms):
                kps.append(dict(xy=(f32(-100), f32(-100)), octave=0, desc=hadamard_desc(253), xright=f32(-1), occupied=0))
            L, K = self._lm_arrays(lms), self._kp_arrays(kps)
            return dict(pos_w=L["pos_w"], valid=L["valid"], min_valid_dist=L["min_valid_dist"], max_valid_dist=L["max_valid_dist"], lm_desc=L["lm_desc"],
                        desc=K["tdesc"], xy=K["t_xy"], octave=K["t_octave"])
        return side(self.lm, kp1), side(lm2, kp2), self.opt.get("cam1", self.cam)

    def expected(self):
        """what `run` has to return where the result is a match list: (match, num) -- for mutually (m21, m12, mutual, num)"""
        e = np.array(self.expect, np.int32).reshape(-1)
        if self.ep != "mutually":
            return e, int((e >= 0).sum())
        kf1, kf2, _ = self.sides()
        e2 = e if self.expect2 is None else np.array(self.expect2, np.int32).reshape(-1)
        m21, m12 = np.full(len(kf1["pos_w"]), -1, np.int32), np.full(len(kf2["pos_w"]), -1, np.int32)
        m21[:len(e)], m12[:len(e2)] = e, e2
        mut = np.array([m if m >= 0 and m12[m] == i else -1 for i, m in enumerate(m21)], np.int32).reshape(-1)
        return m21, m12, mut, int((mut >= 0).sum())

    def level_ties(self):
        """|q - round(q)| of log(max_valid / dist) / log_scale_factor for every landmark whose level is predicted and used"""
        out = []
        if self.ep == "current_last":
            return out
        for lms in (self.lm, self.lm2 or []):
            for i, l in enumerate(lms):
                d = l.get("level_dist", l["dist"])
                if l["valid"] and l["pos"][2] > 0 and np.isfinite(d) and d > 0 and not (lms is self.lm and i in self.exact_level):
                    q = level_q(l["maxv"], d)
                    out.append(abs(q - round(q)))
        return out


def oracle_backend():
    def reproject(cam, R, t, pw, nv, mn, mx, thr, levels, lsf, valid):
        vis, rp, xr, lv = O.can_observe(cam, R, t, pw, nv, mn, mx, thr, levels, lsf)
        vis = vis & (valid != 0)    # a landmark that is not offered: the device's `skip`
        rp[vis == 0], xr[vis == 0], lv[vis == 0] = 0, 0, -1
        return vis, rp, xr, lv
    return dict(cam=oracle_cam, reproject_landmarks=reproject, current_last=O.match_current_and_last_frames,
                frame_keyframe=O.match_frame_and_keyframe_projection, sim3=O.match_by_sim3_transform, mutually=O.match_keyframes_mutually,
                fuse=O.fuse_detect_duplication)


# ================================================================================================================= the classes
def _cam_for(ep, model="perspective", stereo=False):
    return cam_spec(model, 32.0 if stereo else 0.0)


def _spread(i, n_per_row=12):
    """an image point of its own for landmark i: cell centres 80 px apart, clear of each other by more than two margins"""
    return 72.0 + 80.0 * (i % n_per_row), 72.0 + 80.0 * (i // n_per_row)


def _at(img_x, img_y, Z=1.0):
    return np.array([(img_x - CX) * Z / FX, (img_y - CY) * Z / FX, Z])


def image_bounds():
    """project_to_image: rx / ry on min / max -- strict for perspective and fisheye (perspective.cc:146-147, fisheye.cc:185-186), inclusive for
    radial division (radial_division.cc:124-129).  The nine plants of a bound point (three Z, three sides) lie 80 px apart along the bound,
    each private keypoint in a cell of its own.
    The depth test `Z <= 0 fails`: off-axis points at Z == 0, either smallest double and -1, each with a valid-distance range around its
    own distance, so that no other gate rejects them -- at the smallest positive Z the image point is +inf, outside for every model, and
    only the bound tests say so.  Those plants cannot tell `<=` from `<` at Z == 0 (the image point is +inf there too).  The origin
    (0, 0, 0) with min_valid 0 can, through the radial-division camera and reproject_landmarks: were Z == 0 let through, the image point
    would be 0 * inf = NaN, which that model's bound test `!(rx < min || rx > max)` accepts, and distance 0 lies in [0, 1.3]; nothing
    else would reject it.  As the reference stands the depth test rejects it before any NaN is formed, so nothing of it is written
    out.  (0, 0, -smallest) goes with it.  Equirectangular: a point behind the camera is visible."""
    out = []
    tiny = np.nextafter(0.0, 1.0)
    for model in PINHOLE:
        incl = model == "radial_division"
        for ep in ENTRY_POINTS:
            p = Problem("image_bounds", ep, f"{model}", _cam_for(ep, model))
            for axis, (b_lo, b_hi, c) in enumerate(((0.0, float(W), CX), (0.0, float(H), CY))):
                for b in (b_lo, b_hi):
                    j = 0
                    for Z in (1.0, 2.0, 4.0):
                        for side in (-1, 0, 1):
                            v = coord_for(b, side, Z, c)
                            along = _at(72.0 + 80.0 * j, 72.0 + 80.0 * j, Z)[1 - axis]   # a cell centre of its own along the bound
                            j += 1
                            pos = np.array([v, along, Z]) if axis == 0 else np.array([along, v, Z])
                            inside = (side > 0) if b == b_lo else (side < 0)
                            rx, ry, _ = project(*pos)
                            assert (ry if axis == 0 else rx) == 72.0 + 80.0 * (j - 1)
                            # the private keypoint lies in the grid: next to the bound on the inner side (the margin gate is far away)
                            kx, ky = float(np.clip(f32(rx), 2.0 ** -10, W - 2.0 ** -10)), float(np.clip(f32(ry), 2.0 ** -10, H - 2.0 ** -10))
                            p.landmark(pos, expect=inside or (incl and side == 0), kp_xy=(kx, ky))
            for Z in (0.0, -tiny, tiny, -1.0):
                p.landmark(np.array([0.125, 0.125, Z]), expect=False)
            for Z in (0.0, -tiny):
                p.landmark(np.array([0.0, 0.0, Z]), maxv=1.0, minv=0.0, normal=np.array([0.0, 0.0, 1.0]), expect=False)
            out.append(p)
    p = Problem("image_bounds", "reproject_landmarks", "equirectangular", cam_spec("equirectangular", cols=1920, rows=960))
    for pos in ((0.0, 0.0, -2.0), (1.0, 0.5, -2.0), (0.0, 0.0, 2.0), (-1.0, -0.5, -4.0)):
        p.landmark(np.array(pos), kp=None, expect=True)
    out.append(p)
    return out


def _float_bounds(maxv, minv):
    far_, near_ = f32(1.3), f32(1.0 / 1.3)
    return far_ * f32(maxv), near_ * f32(minv)     # float32 products, landmark.h:88-92


def distance_float():
    """dist_mode 0 (frame::can_observe -> landmark::is_inside_in_orb_scale, landmark.h:88-92): (float)dist against (float)1.3 * max_valid and
    (float)(1 / 1.3) * min_valid, both formed in float32, both ends inclusive.  Z is the planted float widened to double.  That alone
    would let a comparison of the double distance pass, so each end also has the double one step OUTSIDE the widened float bound: it
    rounds to the bound as a float and stays visible, where the double comparison would reject it."""
    p = Problem("distance_float", "reproject_landmarks", "perspective", _cam_for(None))
    for maxv, minv in ((f32(2.0), f32(1.0)), (f32(3.3), f32(1.7)), (f32(1.0), f32(0.3))):
        hi, lo = _float_bounds(maxv, minv)
        for b, far in ((hi, True), (lo, False)):
            for side in (-1, 0, 1):
                z = b if side == 0 else np.nextafter(b, f32(-np.inf) if side < 0 else f32(np.inf))
                inside = (side <= 0) if far else (side >= 0)
                p.landmark(np.array([0.0, 0.0, f64(z)]), maxv=maxv, minv=minv, kp=None, expect=inside)
            z = np.nextafter(f64(b), np.inf if far else -np.inf)
            assert f32(z) == b and z != f64(b)
            p.landmark(np.array([0.0, 0.0, z]), maxv=maxv, minv=minv, kp=None, expect=True)
    return [p]


def _double_vs_float_scale():
    """a max_valid whose float bound rejects a distance the double bound accepts (the float product rounds down by more than half an ulp
    of the distance); at max_valid == 1 no such float exists -- 1.3f lies within half an ulp of 1.3 -- so the scale is searched"""
    for k in range(1, 4096):
        maxv = f32(1.0) + f32(k) / f32(4096.0)
        fb, db = f32(1.3) * maxv, f64(1.3) * f64(maxv)
        if f32(db) > fb:      # Z = db: the double test accepts (inclusive), (float)Z is the next float above the float bound
            return maxv
    raise AssertionError("no scale separates the float and the double test")


def distance_double():
    """dist_mode 1 (projection.cc:233-241, 357-365, fuse.cc:52-61): dist against 1.3 * (double)max_valid and (1 / 1.3) * (double)min_valid in
    double, both ends inclusive.  Two landmarks separate the float test of frame::can_observe from this one: `float accepts, double
    rejects` (max_valid 1, Z one double above 1.3: its float is 1.3f == the float bound) and `float rejects, double accepts`
    (max_valid from `_double_vs_float_scale`, Z == the double bound)."""
    out = []
    mv = _double_vs_float_scale()
    for ep in ("frame_keyframe", "sim3", "fuse", "mutually"):
        p = Problem("distance_double", ep, "perspective", _cam_for(ep))
        for maxv, minv in ((f32(2.0), f32(1.0)), (f32(3.3), f32(1.7)), (f32(1.0), f32(0.3))):
            hi, lo = f64(1.3) * f64(maxv), (f64(1.0) / f64(1.3)) * f64(minv)
            for b, far in ((hi, True), (lo, False)):
                for side in (-1, 0, 1):
                    z = b if side == 0 else np.nextafter(b, -np.inf if side < 0 else np.inf)
                    inside = (side <= 0) if far else (side >= 0)
                    # (on the axis, so every private keypoint sits at (cx, cy): the landmarks are told apart by their descriptors alone)
                    p.landmark(np.array([0.0, 0.0, z]), maxv=maxv, minv=minv, expect=inside)
        z = np.nextafter(f64(1.3), np.inf)
        assert f32(z) <= _float_bounds(1.0, 0.3)[0]
        p.landmark(np.array([0.0, 0.0, z]), maxv=1.0, minv=0.3, expect=False)           # float accepts, double rejects
        z = f64(1.3) * f64(mv)
        assert f32(z) > _float_bounds(mv, 0.3)[0]
        p.landmark(np.array([0.0, 0.0, z]), maxv=mv, minv=0.3, expect=True)             # float rejects, double accepts
        out.append(p)
    return out


def no_distance_test():
    """dist_mode 2 (projection.cc:128-135): match_current_and_last_frames has no distance test -- a landmark far outside any range matches.
    (The entry point takes no range at all; the plants hold one so that a kernel which read it would show.)"""
    p = Problem("no_distance_test", "current_last", "perspective", _cam_for(None))
    for i, Z in enumerate((1.0, 2.0, 4.0)):
        x, y = _spread(i)
        p.landmark(_at(x, y, Z), maxv=1e-3, minv=1e-4, level=2, expect=True)
    return [p]


_NZ = (np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0))


def ray_cosine():
    """normal_mode 0 (frame.cc:76-80): on-axis point at a power-of-two Z, ray_cos == nz exactly; `ray_cos < 0.5` fails."""
    p = Problem("ray_cosine", "reproject_landmarks", "perspective", _cam_for(None))
    for Z in (1.0, 2.0, 4.0):
        for nz, ok in zip(_NZ, (False, True, True)):
            p.landmark(np.array([0.0, 0.0, Z]), normal=np.array([0.0, np.sqrt(1 - nz * nz), nz]), kp=None, expect=ok)
    return [p]


def half_dot():
    """normal_mode 1 (projection.cc:370-372, fuse.cc:67-69): `dot(v, normal) < 0.5 * |v|` fails; on the axis dot == Z * nz and |v| == Z."""
    out = []
    for ep in ("sim3", "fuse"):
        p = Problem("half_dot", ep, "perspective", _cam_for(ep))
        for Z in (1.0, 2.0, 4.0):
            for nz, ok in zip(_NZ, (False, True, True)):
                p.landmark(np.array([0.0, 0.0, Z]), normal=np.array([0.0, np.sqrt(1 - nz * nz), nz]), expect=ok)
        out.append(p)
    return out


def no_normal_test():
    """normal_mode 2: match_current_and_last_frames, match_frame_and_keyframe and match_keyframes_mutually have no normal test (their
    interfaces take no normal; the plants carry a back-facing one so that a kernel which read it would show)."""
    out = []
    for ep in ("current_last", "frame_keyframe", "mutually"):
        p = Problem("no_normal_test", ep, "perspective", _cam_for(ep))
        for i, Z in enumerate((1.0, 2.0, 4.0)):
            x, y = _spread(i)
            p.landmark(_at(x, y, Z), normal=np.array([0.0, 0.0, -1.0]), expect=True)
        out.append(p)
    return out


def sim3_center():
    """center_mode 1 (projection.cc:487, 555): match_keyframes_mutually ranges the TRANSFORMED point.  s_12 = 2, identity rot_12,
    trans_12 = (0, 0, 1): a keyframe-1 landmark p maps to p / 2 - (0, 0, 1/2) in keyframe 2, a keyframe-2 landmark to 2 p + (0, 0, 1).
    Keyframe 1 holds (0, 0, 5) -> (0, 0, 2), keyframe 2 holds (0, 0, 1) -> (0, 0, 3); of each pair of landmarks one has a range around
    the transformed distance only (matches) and one around the world distance only (does not).  Every keypoint lies at (cx, cy)."""
    p = Problem("sim3_center", "mutually", "perspective", _cam_for(None), s_12=2.0, trans_12=(0.0, 0.0, 1.0))
    kp1 = []
    for maxv, minv, ok in ((2.2, 1.0, True), (5.5, 4.0, False)):           # [0.77, 2.86] holds 2 only; [3.08, 7.15] holds 5 only
        assert (minv / 1.3 <= 2.0 <= 1.3 * maxv) == ok and (minv / 1.3 <= 5.0 <= 1.3 * maxv) == (not ok)
        i = p.landmark(np.array([0.0, 0.0, 5.0]), maxv=maxv, minv=minv, kp=None, expect=False)
        p.lm[i]["level_dist"] = 2.0
        k = p.keypoint(CX, CY, predict_level(maxv, 2.0), i)
        p.expect[i], p.vis[i] = (k if ok else -1), ok
    s2 = p.second_side()
    for maxv, minv, ok in ((3.3, 2.0, True), (1.1, 0.5, False)):           # [1.54, 4.29] holds 3 only; [0.38, 1.43] holds 1 only
        assert (minv / 1.3 <= 3.0 <= 1.3 * maxv) == ok and (minv / 1.3 <= 1.0 <= 1.3 * maxv) == (not ok)
        i = p.landmark(np.array([0.0, 0.0, 1.0]), maxv=maxv, minv=minv, kp=None, expect=False, **s2)
        p.lm2[i]["level_dist"] = 3.0
        kp1.append(dict(xy=(f32(CX), f32(CY)), octave=predict_level(maxv, 3.0), desc=p.lm2[i]["desc"], xright=f32(-1), occupied=0))
        p.expect2[i] = len(kp1) - 1 if ok else -1
    p.opt["kp1"] = kp1
    return [p]


def _maxv_for_level(dist, l):
    """a range whose predicted level is l, half way between the ties"""
    return f32(dist * np.float64(1.2) ** (l - 0.5)) if l > 0 else f32(dist * 0.9)


def scale_level():
    """landmark::predict_scale_level (landmark.cc:336-353): max_valid / fdist == 1 exactly -> log 0 -> level 0; a ratio just below 1 -> level 0;
    a ratio far above 1.2^num_levels clamps to num_levels - 1; levels 1 .. 6 half way between the ties.  Through a matcher the level shows
    in the window: per level four landmarks, with private keypoints at octaves l - 2, l - 1, l + 1, l + 2 (where they exist), each
    landmark at an image point of its own (`_spread`).  Off the axis the distance is no round number, but the ratio stays exact where
    it has to: max_valid is the float distance itself (ratio 1) or the float below it."""
    def rows(d):   # d: the distance as the kernel's float
        d = f32(d)
        return ([("one", d, 0, True), ("below_one", np.nextafter(d, f32(0)), 0, True), ("clamp", f32(64.0) * d, LEVELS - 1, False),
                 ("clamp_far", f32(1e20), LEVELS - 1, False)] + [(f"level{l}", _maxv_for_level(f64(d), l), l, False) for l in range(1, LEVELS - 1)])
    out = []
    p = Problem("scale_level", "reproject_landmarks", "perspective", _cam_for(None))
    for name, maxv, l, exact in rows(2.0):
        i = p.landmark(np.array([0.0, 0.0, 2.0]), maxv=maxv, minv=1e-30, level=l, kp=None, expect=True)
        if exact:
            p.exact_level.add(i)
    out.append(p)
    for ep in ("frame_keyframe", "sim3", "fuse", "mutually"):
        p = Problem("scale_level", ep, "perspective", _cam_for(ep))
        n = 0
        for k in range(len(rows(2.0))):
            for j in (-2, -1, 1, 2):
                pos = _at(*_spread(n), 2.0)
                name, maxv, l, exact = rows(np.sqrt((pos[0] * pos[0] + pos[1] * pos[1]) + pos[2] * pos[2]))[k]
                if 0 <= l + j < LEVELS:
                    n += 1
                    i = p.landmark(pos, maxv=maxv, minv=1e-30, level=l, kp_octave=l + j, expect=abs(j) <= 1)
                    if exact:
                        p.exact_level.add(i)
        out.append(p)
    return out


def level_window():
    """reproject_window: octaves l - 2 .. l + 2 against [l - 1, l + 1] (window_mode 0), [l, l + 1] (1, assume_forward, projection.cc:141-143)
    and [l - 1, l] (2, :145-147), with l = 0 and l = num_levels - 1 for the clamps.  Modes 1 / 2: match_current_and_last_frames with a
    stereo camera, rot = I, so trans_lc[2] == trans_lw[2]: on true_baseline (strict `>`: mode 0), one double above it (forward), on its
    negation (mode 0) and one double beyond that (backward)."""
    out = []
    tb = 32.0 / FX
    up = float(np.nextafter(f64(f32(tb)), np.inf))
    poses = [("mono", None, 0), ("on_baseline", tb, 0), ("forward", up, 1), ("on_minus_baseline", -tb, 0), ("backward", -up, 2)]
    lo = {0: -1, 1: 0, 2: -1}
    hi = {0: 1, 1: 1, 2: 0}
    for name, tz, mode in poses:
        p = Problem("level_window", "current_last", name, _cam_for(None, stereo=tz is not None), trans_lw=(0.0, 0.0, tz or 0.0), true_baseline=tb)
        i = 0
        for l in (0, 3, LEVELS - 1):
            for o in range(l - 2, l + 3):
                if 0 <= o < LEVELS:
                    x, y = _spread(i)
                    i += 1
                    p.landmark(_at(x, y, 2.0), level=l, kp_octave=o, expect=lo[mode] <= o - l <= hi[mode])
        out.append(p)
    for ep in ("frame_keyframe", "sim3", "fuse", "mutually"):
        p = Problem("level_window", ep, "mode0", _cam_for(ep))
        i = 0
        for l in (0, 3, LEVELS - 1):
            for o in range(l - 2, l + 3):
                if 0 <= o < LEVELS:
                    _ranged(p, ep, _at(*_spread(i), 2.0), l, kp_octave=o, expect=abs(o - l) <= 1)
                    i += 1
        out.append(p)
    return out


def _exact_offset(ref, d):
    """a float32 coordinate k with k - ref == -d exactly in float32 (the subtraction the margin gate performs)"""
    k = f32(ref) - f32(d)
    assert f64(k) == f64(f32(ref)) - f64(f32(d)) and k - f32(ref) == -f32(d), (ref, d)
    return k


def _ranged(p, ep, pos, l, **kw):
    d = float(np.sqrt((pos[0] * pos[0] + pos[1] * pos[1]) + pos[2] * pos[2]))
    return p.landmark(pos, maxv=_maxv_for_level(d, l), minv=1e-3, level=l, **kw)


def margin():
    """k_grid_walk (data/common.cc:127-190): |dx| or |dy| below, on, above margin * scale_factors[l]; strict `<`.  Level 0 (scale factor
    1.0, margin 10) and level 1 (the float32 product 10 * 1.2f used as is).  The reference point is (16, y) or (x, 16) and the keypoint
    lies on its low side, where keypoint - reference == -d holds exactly in float32 (`_exact_offset`)."""
    out = []
    for ep in MATCHERS:
        p = Problem("margin", ep, "perspective", _cam_for(ep), margin=10.0)
        i = 0
        for l in (0, 1):
            m = f32(10.0) * SF[l]
            for axis in (0, 1):
                for side, ok in ((-1, True), (0, False), (1, False)):
                    d = m if side == 0 else np.nextafter(m, f32(-np.inf) if side < 0 else f32(np.inf))
                    other = 72.0 + 80.0 * i
                    i += 1
                    ref = (16.0, other) if axis == 0 else (other, 16.0)
                    k = _exact_offset(16.0, d)
                    _ranged(p, ep, _at(*ref), l, kp_xy=(k, other) if axis == 0 else (other, k), expect=ok)
        out.append(p)
    return out


def window_cells():
    """k_grid_walk's window: reference +- margin exactly on cell edges (margin 8 around a cell centre, level 0), keypoints just inside the
    first and the last cell of the window and just inside the cells beyond; windows clipped at column / row 0 and at the last column /
    row; a window wider than 64 cells (margin 100: the second and later trips of the lane loop) with keypoints in its first, last and
    corner cells; and (match_keyframes_mutually, keyframe 1 of a 512 x 384 camera) a window wholly outside the grid."""
    out = []
    eps_lo = lambda v: np.nextafter(f32(v), f32(-np.inf))
    eps_hi = lambda v: np.nextafter(f32(v), f32(np.inf))
    for ep in MATCHERS:
        p = Problem("window_cells", ep, "edges", _cam_for(ep), margin=8.0)
        rows = []
        for j, (axis, at, ok) in enumerate([(a, f(c), ok) for a, c in ((0, 88.0), (1, 200.0)) for f, ok in
                                            ((lambda c: eps_hi(c - 8), True), (lambda c: eps_lo(c + 8), True), (lambda c: c - 8, False),
                                             (lambda c: c + 8, False), (lambda c: eps_lo(c - 8), False), (lambda c: eps_hi(c + 8), False))]):
            ref = (88.0, 72.0 + 48.0 * j) if axis == 0 else (200.0 + 64.0 * j, 200.0)    # 88 = 16 * 5 + 8, 200 = 16 * 12 + 8: cell centres
            rows.append((ref, (at, ref[1]) if axis == 0 else (ref[0], at), ok))
        # clipped at the four borders: the window reaches beyond the grid, the keypoint lies in the border cell
        rows += [((4.0, 408.0), (1.0, 408.0), True), ((1020.0, 408.0), (1023.0, 408.0), True), ((408.0, 4.0), (408.0, 1.0), True),
                 ((408.0, 764.0), (408.0, 767.0), True), ((4.0, 4.0), (1.0, 1.0), True), ((1020.0, 764.0), (1023.0, 767.0), True)]
        for ref, kxy, ok in rows:
            _ranged(p, ep, _at(*ref), 0, kp_xy=kxy, expect=ok)
        out.append(p)
        p = Problem("window_cells", ep, "wide", _cam_for(ep), margin=100.0)
        for ref, d in (((200.0, 200.0), (-99.0, -99.0)), ((520.0, 200.0), (99.0, 99.0)), ((200.0, 520.0), (99.0, -99.0)), ((520.0, 520.0), (-99.0, 99.0)),
                       ((840.0, 360.0), (0.0, 99.0)), ((840.0, 600.0), (100.0, 0.0))):
            _ranged(p, ep, _at(*ref), 0, kp_xy=(ref[0] + d[0], ref[1] + d[1]), expect=abs(d[0]) < 100 and abs(d[1]) < 100)
        out.append(p)
    # wholly outside: the second pass of match_keyframes_mutually reprojects with keyframe 2's camera (projection.cc:550) and looks up
    # keyframe 1's grid (:571) -- with a smaller keyframe-1 image the window lies beyond the last column / row
    p = Problem("window_cells", "mutually", "outside", _cam_for(None), margin=8.0, cam1=cam_spec("perspective", cols=512, rows=384, cx=256.0, cy=192.0))
    _ranged(p, "mutually", _at(200.0, 200.0), 0, expect=True)                        # keyframe 1 -> 2: an ordinary match
    s2 = p.second_side()
    kp1 = []
    for ref, ok in (((200.0, 200.0), True), ((900.0, 200.0), False), ((200.0, 700.0), False), ((900.0, 700.0), False), ((516.0, 200.0), True)):
        i = _ranged(p, "mutually", _at(*ref), 0, kp=None, expect=False, **s2)
        kx, ky = (min(ref[0], 511.0), min(ref[1], 383.0))
        kp1.append(dict(xy=(f32(kx), f32(ky)), octave=0, desc=p.lm2[i]["desc"], xright=f32(-1), occupied=0))
        if ok:
            p.expect2[i] = len(kp1) - 1
    p.opt["kp1"] = kp1
    out.append(p)
    return out


def stereo_gate():
    """the stereo gate of match_current_and_last_frames (projection.cc:172-177): |x_right - stereo_x_right| below, on, above
    margin * scale_factors[l]; `margin * sf < error` fails, so ON passes.  focal_x_baseline 32, Z 1, reference x 48: x_right == 16 and
    16 - d is exact in float32.  A keypoint with negative x_right, or with x_right == 0 (`> 0` is strict), is not gated at all."""
    p = Problem("stereo_gate", "current_last", "perspective", _cam_for(None, stereo=True), margin=10.0)
    i = 0
    for l in (0, 1):
        m = f32(10.0) * SF[l]
        for side, ok in ((-1, True), (0, True), (1, False)):
            d = m if side == 0 else np.nextafter(m, f32(-np.inf) if side < 0 else f32(np.inf))
            y = 40.0 + 64.0 * i
            i += 1
            pos = _at(48.0, y)
            assert project(*pos, fxb=32.0)[2] == f32(16.0)
            p.landmark(pos, level=l, kp_xright=_exact_offset(16.0, d), expect=ok)
    for xr in (-1.0, -40.0, 0.0):
        y = 40.0 + 64.0 * i
        i += 1
        p.landmark(_at(48.0, y), level=0, kp_xright=xr, expect=True)
    p.landmark(_at(48.0, 40.0 + 64.0 * i), level=0, kp_xright=27.0, expect=False)   # the error's sign does not matter (fabsf)
    return [p]


def _chi_edge(thr32, inv32, base):
    """the two adjacent doubles e (multiples of the step of `base + e`) with  (double)thr < (e * e + 0) * (double)inv  false / true"""
    thr, inv = f64(f32(thr32)), f64(f32(inv32))
    gated = lambda e: thr < (e * e + f64(0.0) * f64(0.0)) * inv
    e = f64(base + np.sqrt(thr / inv)) - f64(base)
    while gated(e):
        e = f64(np.nextafter(base + e, -np.inf)) - f64(base)
    up = f64(np.nextafter(base + e, np.inf)) - f64(base)
    assert not gated(e) and gated(up) and base + e - base == e and base + up - base == up
    return e, up


def _chi_float_square(thr32, inv32):
    """(e_x, d): e_x a multiple of 1/8 and d a float32 in [1, 2) for which the stereo arm's test, with the x_right error d squared in
    float32 as the reference squares it, passes -- and would gate had the square been formed in double.  Searched, not derived: the
    float square has to round down across the threshold."""
    thr, inv = f64(f32(thr32)), f64(f32(inv32))
    for ex in np.arange(0.0, 8.0, 0.125):
        rest = thr / inv - ex * ex
        if not 1.0 < rest < 3.9:
            continue
        d = f32(np.sqrt(rest))
        for _ in range(64):
            d = np.nextafter(d, f32(0))
        for _ in range(128):
            d = np.nextafter(d, f32(np.inf))
            as_float = thr < ((f64(ex) * f64(ex) + f64(0.0) * f64(0.0)) + f64(d * d)) * inv
            as_double = thr < ((f64(ex) * f64(ex) + f64(0.0) * f64(0.0)) + f64(d) * f64(d)) * inv
            if as_double and not as_float:
                return float(ex), d
    raise AssertionError("no x_right error separates the float square from the double square")


def chi_gate():
    """the chi-square gate of fuse::detect_duplication(do_reprojection_matching) (fuse.cc:92-119): e_y == 0, e_x on the two adjacent reachable
    doubles either side of sqrt(threshold / inv_level_sigma_sq): 5.99146f (monocular arm) and 7.81473f (stereo arm, x_right error 0), at
    octave 0 (inv_level_sigma_sq == 1) and octave 1.  Stereo arm also: e_x == 0 and the two adjacent float32 x_right errors either side
    of the threshold; and, per octave, one plant (`_chi_float_square`) that passes only because the square of the x_right error is
    formed in float32 before it is widened.  x_right == 0 is a stereo keypoint here (`>= 0`), a negative one takes the monocular arm."""
    out = []
    for stereo in (False, True):
        p = Problem("chi_gate", "fuse", "stereo" if stereo else "mono", _cam_for(None, stereo=stereo), margin=10.0, reproj=True)
        fxb = 32.0 if stereo else 0.0
        thr = f32(7.81473) if stereo else f32(5.99146)
        i = 0
        for octave in (0, 1):
            inv = INV_SIGMA_SQ[octave]
            for kx in (600.0, 840.0):   # beyond cx: (kx + e) - cx is exact
                for e, ok in zip(_chi_edge(thr, inv, kx), (True, False)):
                    ky = 24.0 + 48.0 * i
                    i += 1
                    pos = _at(kx + e, ky)
                    rx, ry, xr = project(*pos, fxb=fxb)
                    assert rx - f64(f32(kx)) == e and ry == ky
                    # level octave + 1 keeps margin * scale_factor above |e| and the octave inside the window
                    _ranged(p, "fuse", pos, octave + 1, kp_xy=(kx, ky), kp_octave=octave, kp_xright=xr if stereo else -1.0, expect=ok)
        if stereo:
            for octave in (0, 1):
                inv = f64(INV_SIGMA_SQ[octave])
                gated = lambda d: f64(thr) < (f64(0.0) + f64(0.0) + f64(f32(d) * f32(d))) * inv
                d = f32(np.sqrt(f64(thr) / inv))
                while gated(d):
                    d = np.nextafter(d, f32(0))
                while not gated(np.nextafter(d, f32(np.inf))):
                    d = np.nextafter(d, f32(np.inf))
                for dd, ok in ((d, True), (np.nextafter(d, f32(np.inf)), False)):
                    ky = 24.0 + 48.0 * i
                    i += 1
                    pos = _at(36.0, ky)     # x_right == 4: 4 - d is exact in float32
                    assert project(*pos, fxb=fxb)[2] == f32(4.0)
                    _ranged(p, "fuse", pos, octave + 1, kp_octave=octave, kp_xright=_exact_offset(4.0, dd), expect=ok)
                # the square of the x_right error is a FLOAT32 product (fuse.cc:101): a dyadic e_x and a float d with
                #   e_x * e_x + (double)fl32(d * d)  passes  and  e_x * e_x + (double)d * d  would be gated
                ex, d = _chi_float_square(thr, INV_SIGMA_SQ[octave])
                ky = 24.0 + 48.0 * i
                i += 1
                pos = _at(34.0, ky)         # x_right == 2: 2 - d is exact in float32 for d in [1, 2]
                rx, _, xr = project(*pos, fxb=fxb)
                assert xr == f32(2.0) and rx - f64(f32(34.0 - ex)) == ex
                _ranged(p, "fuse", pos, octave + 1, kp_xy=(34.0 - ex, ky), kp_octave=octave, kp_xright=_exact_offset(2.0, d), expect=True)
            # x_right == 0: the stereo arm (error 16: gated); negative: the monocular arm (e == 0: passes)
            for xr, ok in ((0.0, False), (-1.0, True)):
                ky = 24.0 + 48.0 * i
                i += 1
                _ranged(p, "fuse", _at(48.0, ky), 1, kp_octave=0, kp_xright=xr, expect=ok)
        out.append(p)
    return out


def offered():
    """what is offered at all: valid == 0, occupied keypoints, lm_has_observation (two landmarks after one keypoint: the first holds it
    for the second only if it has observations -- the overwrite semantics of curr_frm.add_landmark), empty sides, nothing visible."""
    out = []
    for ep in ENTRY_POINTS:
        p = Problem("offered", ep, "valid", _cam_for(ep))
        for i, (valid, ok) in enumerate(((1, True), (0, False), (1, True), (0, False))):
            x, y = _spread(i)
            p.landmark(_at(x, y, 2.0), valid=valid, expect=ok, kp="own" if ep != "reproject_landmarks" else None)
        out.append(p)
        p = Problem("offered", ep, "nothing_visible", _cam_for(ep))
        for i in range(3):
            p.landmark(np.array([0.125 * i, 0.0, -1.0]), maxv=1.0, expect=False, kp="own" if ep != "reproject_landmarks" else None)
        out.append(p)
        out.append(Problem("offered", ep, "no_landmarks", _cam_for(ep)))
        if ep not in ("reproject_landmarks", "mutually"):
            out[-1].keypoint(100.0, 100.0, 0, 7)
            p = Problem("offered", ep, "no_keypoints", _cam_for(ep))
            p.landmark(_at(200.0, 200.0, 2.0), kp=None, expect=False)
            out.append(p)
    for ep in ("current_last", "frame_keyframe", "sim3"):
        p = Problem("offered", ep, "occupied", _cam_for(ep))
        for i, occ in enumerate((0, 1, 0, 1)):
            x, y = _spread(i)
            p.landmark(_at(x, y, 2.0), occupied=occ, expect=not occ)
        out.append(p)
    for has_obs in (0, 1):
        p = Problem("offered", "current_last", f"has_observation{has_obs}", _cam_for(None))
        a = p.landmark(_at(200.0, 200.0, 2.0), has_obs=has_obs, expect=True)
        p.landmark(_at(200.0, 200.0, 2.0), desc_id=a, kp=p.expect[a], expect=not has_obs)     # the same keypoint again
        out.append(p)
    return out


CLASSES = dict(image_bounds=image_bounds, distance_float=distance_float, distance_double=distance_double, no_distance_test=no_distance_test,
               ray_cosine=ray_cosine, half_dot=half_dot, no_normal_test=no_normal_test, sim3_center=sim3_center, scale_level=scale_level,
               level_window=level_window, margin=margin, window_cells=window_cells, stereo_gate=stereo_gate, chi_gate=chi_gate, offered=offered)

# classes x entry points: what the issue's mode table assigns (tests/test_reproj_problem_classes.py asserts every cell is non-empty)
TABLE = dict(image_bounds=ENTRY_POINTS, distance_float=("reproject_landmarks",), distance_double=("frame_keyframe", "sim3", "fuse", "mutually"),
             no_distance_test=("current_last",), ray_cosine=("reproject_landmarks",), half_dot=("sim3", "fuse"),
             no_normal_test=("current_last", "frame_keyframe", "mutually"), sim3_center=("mutually",),
             scale_level=("reproject_landmarks", "frame_keyframe", "sim3", "fuse", "mutually"), level_window=MATCHERS, margin=MATCHERS,
             window_cells=MATCHERS, stereo_gate=("current_last",), chi_gate=("fuse",), offered=ENTRY_POINTS)

_CACHE = {}


def problems_of(cls):
    if cls not in _CACHE:
        _CACHE[cls] = CLASSES[cls]()
    return _CACHE[cls]


def cells(cls):
    """the (entry point, camera / variant name) pairs of a class, for parametrisation"""
    seen = []
    for p in problems_of(cls):
        if (p.ep, p.cam["model"]) not in seen:
            seen.append((p.ep, p.cam["model"]))
    return seen
