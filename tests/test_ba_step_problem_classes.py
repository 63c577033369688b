"""The one-step bundle-adjustment problems of tests/ba_step_problems.py hold what their classes claim (CPU oracle only, no device): sizes
and block patterns, a step that moved and is not the converged answer, and an oracle reorder spread small enough to carry the tight
bound of tests/test_gpu_ba_step.py."""
import numpy as np
import pytest

from tests import ba_step_problems as B


@pytest.mark.parametrize("name", B.NAMES)
def test_size_and_block_pattern(name):
    p, sc = B.BY_NAME[name], B.scene(name)
    free = B.free_keyframes(sc)
    F = len(free)
    assert F == p["F"] and 6 * F == p["n"]
    assert np.bincount(sc["obs_pose"], minlength=len(sc["pose_fixed"]))[free].min() >= 20  # every free keyframe has its observations
    assert np.bincount(sc["obs_point"], minlength=len(sc["points"])).min() >= 2
    blocks = B.kept_upper_blocks(sc)
    diag = {(a, a) for a in range(F)}
    assert diag <= blocks
    if p["tiled"]:  # AUTO considers the tiled dense LL^T from 24 keyframes on and takes it from 40 % of the upper blocks on
        assert len(sc["pose_fixed"]) >= 24 and F > B.CHOL_LDS_MAX_F
        assert 5 * len(blocks) >= 2 * (F * (F + 1) // 2)
    if p["pattern"] == "blockdiag":
        assert blocks == diag
    if p["pattern"] == "arrow":
        hub = sc["hub_slot"]
        assert hub == (0 if name.endswith("first") else F - 1)
        assert blocks == diag | {(min(hub, a), max(hub, a)) for a in range(F)}
    if p["cls"] == "pcg":  # a chain on each side of the 512 unknowns; the blocks of the smaller one fit the LDS budget
        assert (p["n"] <= B.PCG_LDS_MAX_UNKNOWNS) == (p["pattern"] == "lds")
        assert abs(p["n"] - B.PCG_LDS_MAX_UNKNOWNS) <= 4
        if p["pattern"] == "lds":
            assert B.pcg_lds_bytes(F, len(blocks)) <= B.PCG_LDS_MAX_BYTES
    if p["cls"] == "fixed":
        assert sc["point_fixed"][::7].all() and sc["point_fixed"].sum() == len(sc["points"][::7])
        assert (sc["obs_huber"][::5] == 0).all() and (np.delete(sc["obs_huber"], np.s_[::5]) > 0).all()
    if name == "camera_stereo_f22":
        assert (sc["obs_uvr"][:, 2] >= 0).all() and (sc["intr"][:, 4] > 0).all()
    if name == "camera_equirect_f22":
        assert (sc["intr"][:, :2] == 0).all() and (sc["intr"][:, 2] == 1920).all()


def test_the_size_classes_sit_on_their_boundaries():
    sizes = {c: sorted(p["n"] for p in B.PROBLEMS if p["cls"] == c) for c in ("tiny", "panel", "onchip", "dense", "pcg")}
    assert sizes == dict(tiny=[6, 12, 18], panel=[48, 96], onchip=[126, 132, 138], dense=[144, 150, 192, 228], pcg=[510, 516])
    assert 18 % 16 == 2 and 48 % 16 == 0 and 144 % 48 == 0 and 150 % 48 == 6
    envs = [p["env"] for p in B.PROBLEMS if p["cls"] == "envelope"]
    assert {"SVGPU_SKY_ONE_SIDED": "1"} in envs and {"SVGPU_SKY_SEGMENTS": "0"} in envs and {"SVGPU_SKY_NO_BAND": "1"} in envs
    assert {"SVGPU_SKY_SEGMENTS": "2"} in envs and {"SVGPU_SKY_SEGMENTS": "3"} in envs
    for p in B.PROBLEMS:  # the on-chip LL^T is asked for only where it fits
        assert (("cholesky" in p["solvers"]) == (p["form"] == "local" and p["F"] <= B.CHOL_LDS_MAX_F)) and ("cholesky" in p["solvers"]) == ("cholesky_mfma" in p["solvers"])


@pytest.mark.parametrize("name", B.NAMES)
def test_one_step_moves_is_not_converged_and_has_a_small_reorder_spread(name):
    p, sc = B.BY_NAME[name], B.scene(name)
    ref, spread_pose, spread_points = B.oracle_reference(name)
    print(f"{name}: F = {p['F']}, n = {p['n']}, reorder spread {spread_pose:.2e} on poses, {spread_points:.2e} on points")
    assert ref["iters_stage1"] == 1 and ref["iters_stage2"] == 0
    assert np.abs(ref["pose_cw"] - sc["pose_cw"]).max() > 1e-3  # the step moved ...
    assert ref["chi2_first_step"] < ref["chi2_initial"]         # ... downhill: a trial was accepted
    conv = B.oracle_step(sc, 5, 10) if p["form"] == "local" else B.oracle_step(sc, 10, 0, "global")
    assert np.abs(ref["pose_cw"] - conv["pose_cw"]).max() > 1e-4  # ... and is not where the converged tests look
    assert np.isfinite(spread_pose) and np.isfinite(spread_points)
    assert spread_pose < 1e-12 and spread_points < 1e-12  # else the class is too ill-conditioned for a tight bound: rebuild it
    rev = B.reversed_copy(sc)
    assert np.array_equal(rev["obs_point"][::-1], sc["obs_point"]) and np.array_equal(rev["obs_uvr"][::-1], sc["obs_uvr"])
