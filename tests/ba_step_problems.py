"""One-damped-step bundle-adjustment problems at the size boundaries of the reduced-system solvers (numpy + the CPU oracle only).

A problem is a scene plus ONE Levenberg-Marquardt iteration: `iters1=1, iters2=0` of the local form, `num_iter=1` of the global form.
After one accepted trial the result is x0 [+] dx, so an error of the Schur complement, the right-hand side, the factorisation or the
back-substitution lands on the output undamped -- the converged runs of tests/test_gpu_ba.py correct such an error away.

F = free keyframes, n = 6 F unknowns of the reduced system.  The classes, by the boundary they sit on (ba_plan.h, svgpu.h):
  tiny      F = 1, 2, 3        n = 18 is the first size past one 16-column MFMA panel (a 2-column remainder)
  panel     F = 8, 16          n = 48: exactly three panels; n = 96
  onchip    F = 21, 22, 23     n = 126: last size of the MFMA form; n = 132: two register tiles per thread; n = 138: the first size the
                               register-tile form no longer fits LDS
  dense     F = 24, 25, 32, 38 n = 144: three whole 48-column tiles; n = 150: a 6-column last tile; n = 192; n = 228.  >= 24 keyframes and
                               >= 40 % of the upper blocks really shared (F = 23 too): the tiled dense LL^T is AUTO's choice
  pcg       F = 85, 86         n = 510 / 516, on each side of the 512 unknowns of the PCG inside one workgroup's LDS; a chain of band 2
                               keeps the kept blocks of F = 85 under its LDS budget
  pattern   F = 8              block-diagonal (no landmark shared between two free keyframes); an arrow (one hub shares landmarks with
                               every other free keyframe, the others share none among themselves) with the hub first and last
  envelope  F = 63, global     one-sided, two-sided, segmented with 2 and 3 cuts, and the general kernel (SVGPU_SKY_NO_BAND)
  camera    F = 22             stereo, equirectangular
  fixed     F = 22             every 7th point fixed, every 5th observation without a kernel
Scenes have no outliers and the generators' default noise: the first trial is accepted, the step is a few centimetres.

Every problem also has its reversed-observation copy (`reversed_copy`): the same sums in another order, the oracle's own noise.
"""
import functools

import numpy as np

from oracle import oracle as O
from stella_vslam_amd import synthetic as S

OBS_KEYS = ("obs_pose", "obs_point", "obs_uvr", "obs_inv_sigma_sq", "obs_huber")
SOLVERS = ("auto", "cholesky", "cholesky_mfma", "pcg", "pcg_multi", "dense", "envelope")
PCG_LDS_MAX_UNKNOWNS, PCG_LDS_MAX_BYTES = 512, 150 * 1024  # the in-LDS PCG (svgpu.h: "6 * free poses <= 512", "~150 KB")
CHOL_LDS_MAX_F = 22                                          # the register-tile LL^T fits LDS up to n = 132


def reversed_copy(scene: dict) -> dict:
    out = dict(scene)
    for k in OBS_KEYS:
        out[k] = np.ascontiguousarray(scene[k][::-1])
    return out


def free_keyframes(scene: dict) -> np.ndarray:
    return np.flatnonzero(np.asarray(scene["pose_fixed"]) == 0)


def kept_upper_blocks(scene: dict) -> set:
    """The upper blocks (a <= b, free-keyframe slots in pose order) of the reduced system that hold a term: every diagonal block of a
    free keyframe with an observation of a free landmark, and (a, b) where a free landmark is observed from both."""
    free = free_keyframes(scene)
    slot = np.full(len(scene["pose_fixed"]), -1, np.int64)
    slot[free] = np.arange(len(free))
    pf = scene.get("point_fixed")
    op, ol = np.asarray(scene["obs_pose"]), np.asarray(scene["obs_point"])
    use = slot[op] >= 0
    if pf is not None:
        use &= np.asarray(pf)[ol] == 0
    s, l = slot[op[use]], ol[use]
    vis = np.zeros((int(ol.max()) + 1, len(free)), bool)
    vis[l, s] = True
    co = vis.astype(np.int64).T @ vis.astype(np.int64)
    a, b = np.nonzero(np.triu(co))
    return set(zip(a.tolist(), b.tolist()))


def pcg_lds_bytes(F: int, NB: int) -> int:
    """LDS the in-LDS PCG asks for with NB kept upper blocks of F free keyframes: blocks, diagonal inverses, five vectors, the block rows."""
    n, nent = 6 * F, 2 * NB - F
    return 8 * (36 * NB + 36 * F + 5 * n + 6 * nent + 48) + 4 * ((F + 2) & ~1) + 8 * nent


def _arc(F, num_fixed, num_lm, obs_per_lm, seed, **kw):
    return S.ba_scene(num_kf=F + num_fixed, num_lm=num_lm, obs_per_lm=obs_per_lm, num_fixed=num_fixed, seed=seed, outlier_frac=0.0, **kw)


def _drop_landmarks_with_fewer_than_two(sc):
    cnt = np.bincount(sc["obs_point"], minlength=len(sc["points"]))
    keep_lm = cnt >= 2
    renum = np.cumsum(keep_lm) - 1
    keep = keep_lm[sc["obs_point"]]
    for k in OBS_KEYS:
        sc[k] = np.ascontiguousarray(sc[k][keep])
    sc["obs_point"] = renum[sc["obs_point"]].astype(np.int32)
    sc["points"], sc["points_gt"] = sc["points"][keep_lm], sc["points_gt"][keep_lm]
    return sc


def _one_free_observer(F, seed):
    """3 F keyframes on the arc, the middle one of every three free: a landmark keeps the observations of its fixed keyframes and of ONE
    free keyframe, so no two free keyframes share a landmark -- the reduced system is block-diagonal."""
    sc = S.ba_scene(num_kf=3 * F, num_lm=160 * F, obs_per_lm=6, num_fixed=0, seed=seed, outlier_frac=0.0)
    fixed = (np.arange(3 * F) % 3 != 1).astype(np.uint8)
    sc["pose_fixed"] = fixed
    sc["pose_cw"] = np.where(fixed[:, None] == 1, sc["pose_gt"], sc["pose_cw"])
    is_free = fixed[sc["obs_pose"]] == 0
    chosen = np.full(len(sc["points"]), -1, np.int64)  # the lowest free observer of an even landmark, the highest of an odd one
    for e in np.flatnonzero(is_free):
        l, p = sc["obs_point"][e], sc["obs_pose"][e]
        if chosen[l] < 0 or (p < chosen[l]) == (l % 2 == 0):
            chosen[l] = p
    keep = ~is_free | (chosen[sc["obs_point"]] == sc["obs_pose"])
    for k in OBS_KEYS:
        sc[k] = np.ascontiguousarray(sc[k][keep])
    return _drop_landmarks_with_fewer_than_two(sc)


def _arrow(F, seed, hub_last):
    """The block-diagonal scene plus a hub: one free keyframe that also observes every third landmark of the others."""
    sc = _one_free_observer(F, seed)
    free = free_keyframes(sc)
    hub = int(free[-1] if hub_last else free[0])
    rng = np.random.default_rng(seed + 1)
    seen = np.zeros(len(sc["points"]), bool)
    seen[sc["obs_point"][sc["obs_pose"] == hub]] = True
    lm = np.flatnonzero(~seen)[::3]
    T = sc["pose_gt"][hub].reshape(3, 4)
    fx, fy, cx, cy = sc["intr"][hub][:4]
    pc = sc["points_gt"][lm] @ T[:, :3].T + T[:, 3]
    u, v = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
    ok = (pc[:, 2] > 0.5) & (u > 20) & (u < 732) & (v > 20) & (v < 460)
    lm, u, v = lm[ok], u[ok] + rng.normal(0, 1, ok.sum()), v[ok] + rng.normal(0, 1, ok.sum())
    extra = dict(obs_pose=np.full(len(lm), hub, np.int32), obs_point=lm.astype(np.int32),
                 obs_uvr=np.stack([u, v, np.full(len(lm), -1.0)], 1).astype(np.float32), obs_inv_sigma_sq=np.ones(len(lm), np.float32),
                 obs_huber=np.full(len(lm), sc["obs_huber"][0], np.float32))
    for k in OBS_KEYS:
        sc[k] = np.concatenate([sc[k], extra[k]])
    order = np.argsort(sc["obs_point"], kind="stable")  # landmark-major, as the adaptors deliver it
    for k in OBS_KEYS:
        sc[k] = np.ascontiguousarray(sc[k][order])
    sc["hub_slot"] = F - 1 if hub_last else 0
    return sc


def _fixed_points_and_no_kernel():
    sc = _arc(22, 2, 1200, 6, 109)
    sc["point_fixed"] = (np.arange(len(sc["points"])) % 7 == 0).astype(np.uint8)
    sc["obs_huber"] = sc["obs_huber"].copy()
    sc["obs_huber"][::5] = 0.0
    return sc


def _problem(name, cls, make, F, form="local", env=None, pattern="any", auto="cholesky", plan=None, tiled=False):
    solvers = tuple(s for s in SOLVERS if F <= CHOL_LDS_MAX_F or s not in ("cholesky", "cholesky_mfma")) if form == "local" else ("envelope",)
    return dict(name=name, cls=cls, make=make, F=F, n=6 * F, form=form, env=env or {}, pattern=pattern, auto=auto, plan=plan, tiled=tiled,
                solvers=solvers)


# (three observations per landmark: a band narrow enough for 64 keyframes to be cut into segments, 8 (widest column + 1) <= 63 block rows)
_ENVELOPE_SCENE = functools.lru_cache(None)(lambda: S.ba_scene_large(num_kf=64, num_lm=4000, obs_per_lm=3, outlier_frac=0.0, seed=64))

# name, class, scene, F, ...: `auto` is the solver AUTO resolves to, `plan` the envelope plan kind, `tiled` marks the dense pattern
# (>= 40 % of the upper blocks shared, >= 24 keyframes) that makes the tiled dense LL^T AUTO's choice
PROBLEMS = [
    _problem("tiny_f1", "tiny", lambda: _arc(1, 2, 200, 3, 101), 1),
    _problem("tiny_f2", "tiny", lambda: _arc(2, 2, 200, 4, 102), 2),
    _problem("tiny_f3", "tiny", lambda: _arc(3, 2, 300, 4, 103), 3),
    _problem("panel_f8", "panel", lambda: _arc(8, 2, 500, 5, 104), 8),
    _problem("panel_f16", "panel", lambda: _arc(16, 2, 800, 6, 105), 16),
    _problem("onchip_f21", "onchip", lambda: _arc(21, 3, 1200, 12, 106), 21),
    _problem("onchip_f22", "onchip", lambda: _arc(22, 2, 1200, 12, 107), 22),
    _problem("onchip_f23", "onchip", lambda: _arc(23, 2, 1200, 12, 108), 23, auto="dense", tiled=True),
    _problem("dense_f24", "dense", lambda: _arc(24, 2, 1200, 12, 110), 24, auto="dense", tiled=True),
    _problem("dense_f25", "dense", lambda: _arc(25, 2, 1200, 12, 111), 25, auto="dense", tiled=True),
    _problem("dense_f32", "dense", lambda: _arc(32, 2, 1500, 12, 112), 32, auto="dense", tiled=True),
    _problem("dense_f38", "dense", lambda: _arc(38, 2, 1500, 12, 113), 38, auto="dense", tiled=True),
    _problem("pcg_f85", "pcg", lambda: S.ba_scene_large(num_kf=86, num_lm=2500, obs_per_lm=3, outlier_frac=0.0, seed=85), 85, auto="pcg_lds", pattern="lds"),
    _problem("pcg_f86", "pcg", lambda: S.ba_scene_large(num_kf=87, num_lm=2500, obs_per_lm=3, outlier_frac=0.0, seed=86), 86, auto="envelope"),
    _problem("pattern_blockdiag", "pattern", lambda: _one_free_observer(8, 120), 8, pattern="blockdiag"),
    _problem("pattern_arrow_hub_first", "pattern", lambda: _arrow(8, 121, False), 8, pattern="arrow"),
    _problem("pattern_arrow_hub_last", "pattern", lambda: _arrow(8, 121, True), 8, pattern="arrow"),
    _problem("envelope_one_sided", "envelope", _ENVELOPE_SCENE, 63, "global", {"SVGPU_SKY_ONE_SIDED": "1"}, plan="one-sided"),
    _problem("envelope_two_sided", "envelope", _ENVELOPE_SCENE, 63, "global", {"SVGPU_SKY_SEGMENTS": "0"}, plan="two-sided"),
    _problem("envelope_2_cuts", "envelope", _ENVELOPE_SCENE, 63, "global", {"SVGPU_SKY_SEGMENTS": "2"}, plan="segmented"),
    _problem("envelope_3_cuts", "envelope", _ENVELOPE_SCENE, 63, "global", {"SVGPU_SKY_SEGMENTS": "3"}, plan="segmented"),
    _problem("envelope_no_band", "envelope", _ENVELOPE_SCENE, 63, "global", {"SVGPU_SKY_NO_BAND": "1"}, plan="one-sided"),
    _problem("camera_stereo_f22", "camera", lambda: _arc(22, 2, 1200, 6, 114, stereo=True), 22),
    _problem("camera_equirect_f22", "camera", lambda: _arc(22, 2, 1200, 6, 115, equirect=True), 22),
    _problem("fixed_points_no_kernel_f22", "fixed", _fixed_points_and_no_kernel, 22),
]
NAMES = [p["name"] for p in PROBLEMS]
BY_NAME = {p["name"]: p for p in PROBLEMS}
SKY_ENV = ("SVGPU_SKY_ONE_SIDED", "SVGPU_SKY_SEGMENTS", "SVGPU_SKY_NO_BAND")


@functools.lru_cache(None)
def scene(name: str) -> dict:
    """The problem's scene, built once per process (scene generation dominates the run time); callers must not modify it."""
    return BY_NAME[name]["make"]()


def oracle_step(sc: dict, iters1: int = 1, iters2: int = 0, form: str = "local") -> dict:
    """The oracle's result of the schedule.  chi2_final of the global form is the robust chi2 behind the last iteration (the oracle's own
    "chi2 after" is taken behind its outlier gate, which the global adjuster does not have)."""
    ref = O.local_ba(sc, iters1=iters1, iters2=iters2, want_trace=True)
    st = ref["stats"]
    out = dict(pose_cw=ref["pose_cw"], points=ref["points"], outlier=ref["outlier"], chi2_initial=float(st[0]), chi2_final=float(st[1]),
               iters_stage1=int(st[2]), iters_stage2=int(st[3]), num_gated=int(st[5]), chi2_first_step=float(ref["trace"][0][0]))
    if form == "global":
        out["chi2_final"] = float(ref["trace"][int(st[2]) - 1][0])
    return out


@functools.lru_cache(None)
def oracle_reference(name: str):
    """(the oracle's one-step result, reorder spread on pose entries, reorder spread on points): the spread is max|delta| between the scene
    and its reversed-observation copy, the oracle's own rounding noise on this problem."""
    p, sc = BY_NAME[name], scene(name)
    ref = oracle_step(sc, form=p["form"])
    rev = oracle_step(reversed_copy(sc), form=p["form"])
    return ref, float(np.abs(ref["pose_cw"] - rev["pose_cw"]).max()), float(np.abs(ref["points"] - rev["points"]).max())
