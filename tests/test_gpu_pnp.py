"""svgpu_pnp_compute_pose / svgpu_pnp_ransac[_batch] on the device (tests/pnp_problems.py holds the yardstick).

A hypothesis of a four-point sample is not compared with a restatement: M^T M then has a four-dimensional null space, EPnP uses an
arbitrary basis of it, and what the hypothesis gives depends on that basis (Eigen's, LAPACK's and the device's Jacobi all differ).  So:
 1. compute_pose on over-determined sets with a unique pose against the long double restatement, within 16 x the deviation numpy's own
    fp64 restatement shows on the same class (floored at 1e-12); on 4- and 5-point sets and coplanar landmarks only basis-independent facts.
 2. the RANSAC bookkeeping against the device's own hypotheses: check_inliers recomputed in numpy from the device's poses, the
    reference's strict selection rule applied to the device's own counts and costs, recompute against svgpu_pnp_compute_pose.
 3. the outcome on planted problems that the restatement solves under three bases of the null space.
 4. the error paths.
The bound of a class is 16 x the smaller deviation of numpy's two fp64 forms (LAPACK's decompositions, the Jacobi's), floored at 1e-12.
Measured on an MI355X (largest figures over the sizes 6, 7, 63, 64, 65, 300 of a class; deviation from the long double restatement):
 noise-free   pinhole: LAPACK 2.0e-14, Jacobi 1.8e-14, device 1.6e-14; equirectangular: 1.4e-14, 2.2e-14, device 1.1e-14;
              far: 7.8e-14, 1.6e-15, device 3.6e-15
 1e-3 rad     pinhole: LAPACK 1.0e-2, Jacobi 1.0e-14, device 1.7e-14; equirectangular: 7.9e-3, 1.3e-14, device 8.4e-15;
              far: 8.6e-3, 4.9e-15, device 2.9e-15                                  (bound 1e-12 in every class)
The tests print the figures per class; DESIGN.md section 13."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from tests import pnp_problems as T

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
MARGIN, CAP = 1e-9, 1e-3


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


def _dev(R, t, R0, t0):
    return max(float(np.abs(R - R0).max()), float(np.abs(t - t0).max() / max(1.0, np.abs(t0).max())))


# ------------------------------------------------------------------------------------------------ 1. compute_pose
@pytest.mark.parametrize("noise", [0.0, 1e-3])
def test_pose_of_overdetermined_sets_against_the_long_double_restatement(ctx, noise):
    from stella_vslam_amd import solve
    sets = T.pose_sets(noise)
    off, brg, pw, _ = T.concatenate(sets)
    pose, err = solve.compute_pose(ctx, brg, pw, off)
    classes = {}
    for k, p in enumerate(sets):
        R, t, e, sv = T.compute_pose(p["bearings"], p["pos_w"])
        if T.null_gap(sv) < 1e-6:
            continue
        Rl, tl, _, _ = T.compute_pose(p["bearings"], p["pos_w"], dtype=np.longdouble)
        Rj, tj, _, _ = T.compute_pose(p["bearings"], p["pos_w"], jacobi=True)
        c = classes.setdefault((p["name"].split("_")[0], len(p["pos_w"])), dict(lapack=0.0, jacobi=0.0, device=0.0, n=0))
        c["lapack"] = max(c["lapack"], _dev(R, t, Rl, tl))
        c["jacobi"] = max(c["jacobi"], _dev(Rj, tj, Rl, tl))
        c["device"] = max(c["device"], _dev(pose[k, :, :3], pose[k, :, 3], Rl, tl))
        c["n"] += 1
        e = T.reprojection_error(pose[k, :, :3], pose[k, :, 3], p["bearings"], p["pos_w"])
        assert abs(err[k] - e) <= 1e-12 * abs(e), (p["name"], err[k], e)
    assert sum(c["n"] for c in classes.values()) >= 0.9 * len(sets)
    bad = []
    for key, c in sorted(classes.items()):
        # numpy's fp64 restatement in its two forms (LAPACK's decompositions, the Jacobi's): the smaller deviation sets the bound.  On noisy
        # sets LAPACK's differs at the level of the noise (the sign of a PCA axis moves the control points), which would bound nothing.
        tol = max(16.0 * min(c["lapack"], c["jacobi"]), 1e-12)
        print(f"noise {noise:g} {key[0]} n={key[1]}: {c['n']} sets, numpy deviation LAPACK {c['lapack']:.3e} Jacobi {c['jacobi']:.3e}, tolerance {tol:.3e}, "
              f"device deviation {c['device']:.3e}")
        if not c["device"] <= tol:
            bad.append((key, c["device"], tol))
    assert not bad, bad


@pytest.mark.parametrize("kind,n", [(k, n) for k in T.KINDS for n in (4, 5)] + [("coplanar", 64), ("coplanar", 300)])
def test_basis_independent_facts_of_minimal_and_coplanar_sets(ctx, kind, n):
    from stella_vslam_amd import solve
    sets = [T.planted(40 + s, n, kind) for s in range(6)]
    off, brg, pw, _ = T.concatenate(sets)
    pose, err = solve.compute_pose(ctx, brg, pw, off)
    for k, p in enumerate(sets):
        R, t = pose[k, :, :3], pose[k, :, 3]
        if not np.isfinite(pose[k]).any():
            continue  # the whole pose is non-finite: no N gave a comparable error
        assert np.isfinite(pose[k]).all()
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1.0) < 1e-9, (p["name"], R)
        e = T.reprojection_error(R, t, p["bearings"], p["pos_w"])
        assert abs(err[k] - e) <= 1e-12 * abs(e), (p["name"], err[k], e)


def test_one_call_with_several_sets_equals_the_single_set_calls(ctx):
    from stella_vslam_amd import solve
    sets = [T.planted(60 + n, n, T.KINDS[n % 4], noise=1e-3) for n in (4, 5, 7, 63, 64, 65, 300)]
    off, brg, pw, _ = T.concatenate(sets)
    pose, err = solve.compute_pose(ctx, brg, pw, off)
    for k, p in enumerate(sets):
        ps, es = solve.compute_pose(ctx, p["bearings"], p["pos_w"])
        assert ps[0].tobytes() == pose[k].tobytes() and es.tobytes() == err[k:k + 1].tobytes(), p["name"]


# ------------------------------------------------------------------------------------------------ 2. RANSAC bookkeeping
def _run_batch(ctx, probs, min_num_inliers=10, recompute=False, with_hypotheses=True):
    from stella_vslam_amd import solve
    off, brg, pw, octv = T.concatenate(probs)
    smp = np.stack([p["samples"] for p in probs])
    return off, solve.pnp_ransac_batch(ctx, off, brg, pw, octv, T.orb_scale_factors(), smp, min_num_inliers, recompute, 10, with_hypotheses)


@pytest.mark.parametrize("k", [1, 3, 17])
def test_bookkeeping_against_the_devices_own_hypotheses(ctx, k):
    probs = T.ransac_batch(k)
    off, out = _run_batch(ctx, probs)
    total = excused = 0
    for j, p in enumerate(probs):
        n = len(p["pos_w"])
        a, b = off[j], off[j + 1]
        if n < 4 or n < 10:
            assert out["valid"][j] == 0 and out["best_iter"][j] == -1 and not out["is_inlier"][a:b].any() and not out["pose_cw"][j].any()
            continue
        mce = T.max_cos_errors(p["octaves"], p["scale_factors"])
        flags_of = []
        for it in range(out["hyp_pose"].shape[1]):
            H = out["hyp_pose"][j, it]
            flags, num, cost, margin = T.check_inliers(H[:, :3], H[:, 3], p["bearings"], p["pos_w"], mce)
            flags_of.append(flags)
            total += n
            # matches the device may have judged the other way: those within MARGIN of their threshold.  The count may differ by at most
            # their number (each difference counts against the cap), the cost by at most their |cos_angle - max_cos_error| beside 1e-12.
            near = margin < MARGIN
            differ = abs(num - int(out["hyp_num_inliers"][j, it]))
            assert differ <= int(near.sum()), (p["name"], it, num, out["hyp_num_inliers"][j, it])
            excused += differ
            slack = float((margin[near] * np.abs(mce[near].astype(np.float64))).sum()) if differ else 0.0
            assert abs(cost - out["hyp_cost"][j, it]) <= 1e-12 * abs(cost) + slack, (p["name"], it, cost, out["hyp_cost"][j, it])
        best = T.select(out["hyp_num_inliers"][j], out["hyp_cost"][j], 10)
        assert out["best_iter"][j] == best and bool(out["valid"][j]) == (best >= 0), (p["name"], best, out["best_iter"][j])
        if best >= 0:
            assert out["pose_cw"][j].tobytes() == out["hyp_pose"][j, best].tobytes()
            diff = out["is_inlier"][a:b].astype(bool) != flags_of[best]
            m = T.check_inliers(out["pose_cw"][j][:, :3], out["pose_cw"][j][:, 3], p["bearings"], p["pos_w"], mce)[3]
            assert (m[diff] < MARGIN).all(), p["name"]
            excused += int(diff.sum())
            assert int(out["is_inlier"][a:b].sum()) == out["hyp_num_inliers"][j, best]
        else:
            assert not out["is_inlier"][a:b].any() and not out["pose_cw"][j].any()
    print(f"batch of {k}: {excused} of {total} match judgements used the margin exemption")
    assert excused <= CAP * max(total, 1), (excused, total)
    assert out["valid"].any()


def test_single_problem_call_equals_the_batch_of_one(ctx):
    from stella_vslam_amd import solve
    p = T.ransac_batch(1)[0]
    _, b = _run_batch(ctx, [p], recompute=True)
    s = solve.pnp_ransac(ctx, p["bearings"], p["pos_w"], p["octaves"], T.orb_scale_factors(), p["samples"], 10, True, 10, True)
    for key in b:
        assert b[key].tobytes() == s[key].tobytes(), key


def test_first_of_equal_costs_wins(ctx):
    """Hand-built tables in which the tie IS the winner: every iteration after the first draws the same four planted inliers, the first
    either draws them too (the winner is iteration 0) or a sample with planted outliers (iteration 0 loses or is not eligible, the winner
    is iteration 1, the first of the identical ones).  A `>=` in the selection would end on the last iteration."""
    probs, first_dup = [], []
    for j in range(8):
        p = T.planted(70 + j, 80, T.KINDS[j % len(T.KINDS)], outliers=0.2)
        inl, outl = np.flatnonzero(~p["planted_outlier"]), np.flatnonzero(p["planted_outlier"])
        good = inl[[1 + j, 11 + j, 23 + j, 37 + j]].astype(np.uint32)
        smp = np.tile(good, (8, 1))
        if j % 2:
            smp[0] = [outl[0], outl[1], inl[0], outl[2]]
        p["samples"] = smp
        probs.append(p)
        first_dup.append(j % 2)
    _, out = _run_batch(ctx, probs)
    eligible = [0, 0]  # ties that won, by the index of their first iteration (whether a four-point hypothesis is good depends on the null-space basis)
    for j, f in enumerate(first_dup):
        num, cost = out["hyp_num_inliers"][j], out["hyp_cost"][j]
        assert (cost[f:] == cost[f]).all() and (num[f:] == num[f]).all() and all(out["hyp_pose"][j, it].tobytes() == out["hyp_pose"][j, f].tobytes() for it in range(f, 8))
        if not num[f] > 10:
            continue
        if f == 1 and num[0] > 10 and cost[0] <= cost[1]:
            continue  # (the contaminated sample happened to do as well: not a tie among the winners)
        eligible[f] += 1
        assert out["valid"][j] == 1 and out["best_iter"][j] == f, (j, f, out["best_iter"][j], num, cost)
    print(f"ties that won: {eligible[0]} starting at iteration 0, {eligible[1]} starting at iteration 1")
    assert eligible[0] >= 1 and eligible[1] >= 1, eligible


def test_recompute_equals_compute_pose_on_the_winners_inliers(ctx):
    from stella_vslam_amd import solve
    probs = T.ransac_batch(17)
    off, plain = _run_batch(ctx, probs, recompute=False)
    _, rec = _run_batch(ctx, probs, recompute=True)
    for key in ("valid", "best_iter", "is_inlier", "hyp_cost"):
        assert plain[key].tobytes() == rec[key].tobytes(), key
    checked = 0
    for j, p in enumerate(probs):
        if not rec["valid"][j]:
            assert rec["pose_cw"][j].tobytes() == plain["pose_cw"][j].tobytes()
            continue
        inl = rec["is_inlier"][off[j]:off[j + 1]].astype(bool)
        pose, _ = solve.compute_pose(ctx, p["bearings"][inl], p["pos_w"][inl])
        assert pose[0].tobytes() == rec["pose_cw"][j].tobytes(), p["name"]
        checked += 1
    assert checked >= 5


def test_no_hypothesis_passes_min_num_inliers(ctx):
    p = T.planted(4, 80, "pinhole", outliers=0.2)
    p["samples"] = T.draw_samples(np.random.default_rng(1), 80, 6)
    _, out = _run_batch(ctx, [p], min_num_inliers=80, recompute=True)
    assert out["valid"][0] == 0 and out["best_iter"][0] == -1 and not out["is_inlier"].any() and not out["pose_cw"].any()


# ------------------------------------------------------------------------------------------------ 3. outcome
def test_planted_problems_end_on_the_planted_inliers(ctx):
    kept, probs = T.outcome_problems()
    assert len(kept) >= 0.9 * len(probs)
    _, out = _run_batch(ctx, probs, with_hypotheses=False)
    off = np.concatenate([[0], np.cumsum([80] * len(probs))])
    total = excused = 0
    for j in kept:
        p = probs[j]
        assert out["valid"][j] == 1, p["name"]
        diff = out["is_inlier"][off[j]:off[j + 1]].astype(bool) != p["planted_flags"]
        mce = T.max_cos_errors(p["octaves"], p["scale_factors"])
        m = np.minimum(p["planted_margin"], T.check_inliers(out["pose_cw"][j][:, :3], out["pose_cw"][j][:, 3], p["bearings"], p["pos_w"], mce)[3])
        assert (m[diff] < MARGIN).all(), (p["name"], np.flatnonzero(diff), m[diff])
        total, excused = total + 80, excused + int(diff.sum())
    assert excused <= CAP * total


# ------------------------------------------------------------------------------------------------ 4. error paths
def _raw_batch(ctx, off, brg, pw, octv, smp, num_levels=8, min_inl=10):
    from stella_vslam_amd._lib import lib
    off, brg, pw, octv, smp = (np.ascontiguousarray(off, np.int32), np.ascontiguousarray(brg, np.float64), np.ascontiguousarray(pw, np.float64),
                               np.ascontiguousarray(octv, np.int32), np.ascontiguousarray(smp, np.uint32))
    k, sf = len(off) - 1, T.orb_scale_factors()
    valid, pose, inl, best = np.zeros(max(k, 1), np.uint8), np.zeros((max(k, 1), 12)), np.zeros(max(len(brg), 1), np.uint8), np.zeros(max(k, 1), np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    return lib().svgpu_pnp_ransac_batch(ctx.handle, k, P(off), P(brg), P(pw), P(octv), P(sf), num_levels, min_inl, smp.shape[1] if smp.ndim == 3 else 0, P(smp), 0,
                                        10, P(valid), P(pose), P(inl), P(best), None, None, None)


def test_invalid_arguments_are_refused_before_any_launch(ctx):
    from stella_vslam_amd._lib import lib
    p, q = T.planted(1, 20, "pinhole"), T.planted(2, 30, "pinhole")
    off, brg, pw, octv = T.concatenate([p, q])
    smp = np.stack([T.draw_samples(np.random.default_rng(3), 20, 4), T.draw_samples(np.random.default_rng(4), 20, 4)])
    assert _raw_batch(ctx, off, brg, pw, octv, smp) == 0
    bad = octv.copy()
    bad[7] = 8
    assert _raw_batch(ctx, off, brg, pw, bad, smp) == 1          # octave outside [0, num_levels)
    bad[7] = -1
    assert _raw_batch(ctx, off, brg, pw, bad, smp) == 1
    s = smp.copy()
    s[0, 1, 2] = 20                                                # index outside its problem (valid in the next one)
    assert _raw_batch(ctx, off, brg, pw, octv, s) == 1
    s = smp.copy()
    s[1, 3, 0] = s[1, 3, 3]                                        # repeated index within one sample
    assert _raw_batch(ctx, off, brg, pw, octv, s) == 1
    assert _raw_batch(ctx, [0, 30, 20], brg, pw, octv, smp) == 1   # non-monotone offsets
    assert _raw_batch(ctx, [0], brg, pw, octv, smp) == 0           # num_problems == 0
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    pose, err = np.zeros((2, 12)), np.zeros(2)
    assert lib().svgpu_pnp_compute_pose(ctx.handle, 2, P(np.array([0, 30, 20], np.int32)), P(brg), P(pw), 10, P(pose), P(err)) == 1
    assert lib().svgpu_pnp_compute_pose(ctx.handle, 2, P(np.array([0, 3, 50], np.int32)), P(brg), P(pw), 10, P(pose), P(err)) == 1
    assert lib().svgpu_pnp_compute_pose(ctx.handle, 0, None, None, None, 10, None, None) == 0
    assert lib().svgpu_pnp_compute_pose(None, 1, P(off), P(brg), P(pw), 10, P(pose), P(err)) == 1


def test_profile_knows_the_kernel_classes():
    from stella_vslam_amd._lib import lib
    L = lib()
    names = L.svgpu_profile_kernels().decode().split(",")
    assert {"k_pnp_pose", "k_pnp_ransac", "k_pnp_select"} <= set(names)


def test_drop_in_class_is_reproducible_and_its_batch_form_equals_the_single_solvers():
    """host/drop_in/pnp_solver_hip: use_fixed_seed gives the same result solver after solver, find_via_ransac_batch equals the single calls."""
    exe = ROOT / "stella_vslam_amd" / "host" / "test_pnp_solver"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pnp_solver ok" in out.stdout
