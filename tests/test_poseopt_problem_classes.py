"""The pose-optimiser problems of tests/poseopt_problems.py hold what their classes claim (CPU oracle only, no device): every gate plant has
exactly its planted residual under the oracle's own edge code, its chi2 lies on the claimed side of its threshold and the oracle flags it
as claimed; every step problem takes one accepted step towards the true pose, stays clear of the gate, and the oracle's step agrees with a
plain numpy longdouble restatement within the oracle's own reorder spread times the project's factor (tests/test_gpu_ba_step.py::K_SPREAD)."""
import numpy as np
import pytest

from tests import poseopt_problems as P

K_SPREAD = 1024


@pytest.mark.parametrize("name", P.GATE_NAMES)
def test_every_plant_has_its_residual_its_side_and_its_flag_under_the_oracle(name):
    p = P.gate_by_name(name)
    n = len(p["pos_w"])
    assert np.array_equal(p["pose_cw"].reshape(3, 4)[:, :3], np.eye(3))
    for i in range(n):   # the oracle's edge sees the planted double, bit for bit
        err, D = P.oracle_edge(p, i)
        assert D == (2 if p["uvr"][i, 2] < 0 else 3), (name, i)
        assert np.array_equal(err, p["residual"][i]), (name, i, err, p["residual"][i])
    planted = P.planted_flags(p)
    assert np.array_equal(planted, p["claim"]), (name, np.flatnonzero(planted != p["claim"]))
    for schedule in P.GATE_SCHEDULES:
        for reverse in (False, True):
            nv, pose, flags, iters = P.oracle_run(p, schedule, reverse)
            assert iters == 0 and np.array_equal(pose, p["pose_cw"]), (name, schedule)
            assert np.array_equal(flags, planted), (name, schedule, np.flatnonzero(flags != planted))
            assert nv == (n - int(planted.sum()) if n >= 5 else 0)


def test_chi_on_threshold_sits_on_the_threshold_and_its_neighbours_beside_it():
    p = P.gate_by_name("chi_on_threshold")
    chi = P.chi2_numpy(p["residual"], p["inv_sigma_sq"]).reshape(-1, 3)
    thr = np.array([float(P.threshold(r)) for r in p["uvr"][:, 2]]).reshape(-1, 3)
    assert len(chi) == 5   # u, v of a monocular edge; u, v, right of a stereo edge
    assert (chi[:, 1] == thr[:, 1]).all() and (chi[:, 0] < thr[:, 0]).all() and (chi[:, 2] > thr[:, 2]).all()
    assert np.array_equal(p["claim"].reshape(-1, 3), np.tile([0, 0, 1], (5, 1)))
    w = p["inv_sigma_sq"].reshape(-1, 3)
    assert (np.nextafter(w[:, 0], np.float32(np.inf)) == w[:, 1]).all() and (np.nextafter(w[:, 1], np.float32(np.inf)) == w[:, 2]).all()
    comps = [tuple(np.flatnonzero(r)) for r in p["residual"][::3]]
    assert comps == [(0,), (1,), (0,), (1,), (2,)] and (np.abs(p["residual"]).sum(1) == 2.0).all()
    assert ((p["uvr"][:, 2] < 0) == np.repeat([True, True, False, False, False], 3)).all()


def test_float_threshold_plants_flip_under_the_double_literal_and_only_those():
    p = P.gate_by_name("float_threshold")
    chi = P.chi2_numpy(p["residual"], p["inv_sigma_sq"])
    assert (p["inv_sigma_sq"] == 1.0).all() and ((p["residual"] != 0).sum(1) == 1).all()
    inside = np.array([t["inside"] for t in p["tags"]])
    mono = p["uvr"][:, 2] < 0
    as_float = np.where(mono, float(P.THR_MONO), float(P.THR_STEREO)) < chi
    as_double = np.where(mono, P.THR_MONO_DOUBLE, P.THR_STEREO_DOUBLE) < chi
    assert np.array_equal(as_float != as_double, inside)
    assert np.array_equal(as_float, p["claim"] != 0)
    assert inside[mono].sum() == 6 and inside[~mono].sum() == 3 and (~inside[mono]).sum() == 4 and (~inside[~mono]).sum() == 2
    assert as_float[inside & mono].all() and not as_float[inside & ~mono].any()   # 5.99146f < 5.99146 and 7.81473 < 7.81473f
    assert np.abs(np.float64(P.THR_MONO) - P.THR_MONO_DOUBLE) < 2e-7 and np.abs(np.float64(P.THR_STEREO) - P.THR_STEREO_DOUBLE) < 2e-7


def test_threshold_choice_is_decided_by_the_edge_kind_alone():
    p = P.gate_by_name("threshold_choice")
    chi = P.chi2_numpy(p["residual"], p["inv_sigma_sq"])
    assert (chi == 7.0).all() and float(P.THR_MONO) < 7.0 < float(P.THR_STEREO)
    mono = p["uvr"][:, 2] < 0
    assert np.array_equal(p["claim"] != 0, mono) and mono.sum() == 6 and (~mono).sum() == 7
    assert p["uvr"][-1, 2] == 0 and np.signbit(p["uvr"][-1, 2]) and p["claim"][-1] == 0


def test_weight_widening_pairs_are_one_ulp_of_e_apart_around_the_threshold():
    from oracle import oracle as O
    p = P.gate_by_name("weight_widening")
    inv = O.scale_tables(1.2, 8)[3]
    e = np.abs(p["residual"]).sum(1).reshape(7, 2)
    w = p["inv_sigma_sq"].reshape(7, 2)
    assert np.array_equal(w[:, 0], inv[1:]) and np.array_equal(w[:, 1], inv[1:])
    assert all(np.frexp(float(x))[0] != 0.5 for x in inv[1:])   # no level's weight is a power of two
    assert np.array_equal(np.nextafter(e[:, 0], np.inf), e[:, 1])
    chi = P.chi2_numpy(p["residual"], p["inv_sigma_sq"]).reshape(7, 2)
    thr = np.array([float(P.threshold(r)) for r in p["uvr"][:, 2]]).reshape(7, 2)
    assert (chi[:, 0] <= thr[:, 0]).all() and (thr[:, 1] < chi[:, 1]).all()
    assert np.array_equal(p["claim"].reshape(7, 2), np.tile([0, 1], (7, 1)))
    assert (thr[:, 0] == float(P.THR_MONO)).sum() == 4 and (thr[:, 0] == float(P.THR_STEREO)).sum() == 3
    # a float product e e w, or w narrowed, would move chi2 by far more than the step between the two plants
    assert (np.abs((e[:, 0] * e[:, 0]).astype(np.float32).astype(np.float64) * w[:, 0] - chi[:, 0]) > 100 * (chi[:, 1] - chi[:, 0])).all()


def test_sizes_plant_an_outlier_at_both_ends_of_every_stride_pass():
    assert P.SIZES == (5, 63, 64, 65, 511, 512, 513, 1024, 1025, 1537)
    assert P.stride_outliers(1537) == [0, 511, 512, 1023, 1024, 1535, 1536] and P.stride_outliers(513) == [0, 511, 512] and P.stride_outliers(64) == [0, 63]
    for n in P.SIZES:
        p = P.gate_by_name(f"size_{n}")
        chi = P.chi2_numpy(p["residual"], p["inv_sigma_sq"])
        out = P.stride_outliers(n)
        assert len(chi) == n and np.array_equal(np.flatnonzero(chi), out) and (chi[out] == 64.0).all()
        assert np.array_equal(np.flatnonzero(p["claim"]), out)
        assert (p["uvr"][:, 2] < 0).any() and (p["uvr"][:, 2] >= 0).any()
    few4, few5 = P.gate_by_name("few_4"), P.gate_by_name("few_5")
    assert len(few4["pos_w"]) == 4 and (P.chi2_numpy(few4["residual"], few4["inv_sigma_sq"]) > 60).sum() == 3 and not few4["claim"].any()
    assert len(few5["pos_w"]) == 5 and few5["claim"].tolist() == [0, 0, 1, 0, 0]


def test_the_batch_form_moves_every_planted_entry_and_holds_the_three_skipped_kinds():
    for group in P.cameras(P.gate_problems()):
        args, members = P.batch_of(group, 7)
        names = [m[0] for m in members]
        assert sorted(n for n in names if n) == sorted(p["name"] for p in group) and names.count(None) == 3
        assert len(group) == 1 or names != [p["name"] for p in group] + [None] * 3   # shuffled
        kinds = set()
        for name, sl, select, active, pose in members:
            assert len(select) == sl.stop - sl.start and np.array_equal(args["select"][sl], select)
            if name is None:
                kinds.add("empty" if len(select) == 0 else "inactive" if not active else "under5" if select.sum() == 4 else "?")
                continue
            p = P.gate_by_name(name)
            keep = select != 0
            assert select[0] == 0 and (~keep).sum() >= 1 and keep.sum() == len(p["pos_w"])   # compaction moves every entry of the problem
            for k in P.OBS_KEYS:
                assert np.array_equal(args[k][sl][keep], p[k])
            # an unselected entry would be an outlier, were it selected
            junk = dict(p, **{k: args[k][sl][~keep] for k in P.OBS_KEYS})
            r, _, _ = P.residuals_numpy(p["pose_cw"], junk)
            assert (P.chi2_numpy(r, junk["inv_sigma_sq"]) > 1000).all()
        assert kinds == {"empty", "inactive", "under5"}


# ------------------------------------------------------------------------------------------- one damped step

def test_the_step_classes_are_what_they_say():
    assert P.STEP_SIZES == (5, 6, 64, 65, 512, 513, 1025)
    for n in P.STEP_SIZES:
        assert len(P.step_problem(f"size_{n}")["pos_w"]) == n
    mono = lambda name: P.step_problem(name)["uvr"][:, 2] < 0
    assert mono("mono").all() and not mono("stereo").any() and mono("equirect").all() and 70 <= mono("mixed").sum() <= 80
    assert (P.step_problem("equirect")["intr"][:2] == 0).all() and P.step_problem("stereo")["intr"][4] > 0
    h = P.step_problem("no_kernel_third")["huber"]
    assert (h[::3] <= 0).all() and (h[::6] == 0).all() and (h[3::6] < 0).all() and (np.delete(h, np.s_[::3]) > 0).all()
    # the planted third lies at 2 .. 4 delta^2 at the initial pose and every other edge below delta^2: both branches of the kernel enter H and b
    p = P.step_problem("huber_planted")
    chi, _ = P.gate_chi2_after(p, p["pose_cw"])
    d2 = p["huber"].astype(np.float64) ** 2
    assert p["planted"].sum() == 50
    assert (chi[p["planted"]] > 1.99 * d2[p["planted"]]).all() and (chi[p["planted"]] < 4.01 * d2[p["planted"]]).all()
    assert (chi[~p["planted"]] < d2[~p["planted"]]).all()
    (nv, pose, flags, iters), _ = P.step_reference("huber_planted", "huber")
    assert flags[p["planted"]].all()   # outliers-to-be
    for name in P.STEP_NAMES:   # elsewhere the initial pose puts edges on both sides of delta^2 by itself
        if name != "huber_planted" and len(P.step_problem(name)["pos_w"]) >= 64:
            q = P.step_problem(name)
            chi, _ = P.gate_chi2_after(q, q["pose_cw"])
            over = chi > q["huber"].astype(np.float64) ** 2
            assert over.sum() >= 5 and (~over).sum() >= 5, name


@pytest.mark.parametrize("mode", list(P.STEP_SCHEDULES))
@pytest.mark.parametrize("name", P.STEP_NAMES)
def test_one_step_is_accepted_moves_towards_the_truth_and_stays_clear_of_the_gate(name, mode):
    p = P.step_problem(name)
    (nv, pose, flags, iters), spread = P.step_reference(name, mode)
    n = len(p["pos_w"])
    assert iters == 1
    moved, before, after = np.abs(pose - p["pose_cw"]).max(), np.linalg.norm(p["pose_cw"] - p["pose_gt"]), np.linalg.norm(pose - p["pose_gt"])
    assert moved > p["min_move"] and after < before, (moved, before, after)
    # the initial pose is a few centimetres and tenths of a degree off
    T0, Tg = p["pose_cw"].reshape(3, 4), p["pose_gt"].reshape(3, 4)
    angle = np.degrees(np.arccos(np.clip((np.trace(T0[:, :3] @ Tg[:, :3].T) - 1) / 2, -1, 1)))
    assert 0.05 <= angle <= 0.5 and 4e-3 <= np.linalg.norm(T0[:, 3] - Tg[:, 3]) <= 0.06
    for rev in (False, True):   # no edge's gate is decided by rounding, in either observation order
        pose_r = P.oracle_run(p, P.STEP_SCHEDULES[mode], reverse=rev)[1]
        chi, thr = P.gate_chi2_after(p, pose_r)
        chi_oracle = P.oracle_chi2(p, pose_r)   # the clearance holds for the oracle's own residuals, and numpy restates them
        assert (np.abs(chi_oracle - thr) > 1e-9 * thr).all() and (np.abs(chi - thr) > 1e-9 * thr).all()
        assert np.abs(chi - chi_oracle).max() <= 1e-11 * max(1.0, chi_oracle.max())
        assert np.array_equal((thr < chi_oracle).astype(np.uint8), flags)
        assert np.array_equal((thr < chi).astype(np.uint8), flags) and nv == n - int(flags.sum())
    assert 0 <= spread < 1e-12, spread   # (0: five terms can sum alike in both orders; the bound then rests on its floor of 64 ulp)
    print(f"{name} {mode}: n {n} num_valid {nv} moved {moved:.2e} |T - T_gt| {before:.2e} -> {after:.2e} reorder spread {spread:.2e}")


@pytest.mark.parametrize("mode", list(P.STEP_SCHEDULES))
@pytest.mark.parametrize("name", P.STEP_NAMES)
def test_the_oracle_step_agrees_with_the_longdouble_restatement(name, mode):
    p = P.step_problem(name)
    (nv, pose, flags, iters), spread = P.step_reference(name, mode)
    restated, dx, chi_before, chi_after = P.restate_step(p, robust=mode == "huber")
    assert chi_after < chi_before   # the trial the restatement takes is an accepted one
    tol = max(K_SPREAD * spread, 64 * float(np.spacing(np.abs(pose).max())))
    d = float(np.abs(restated - pose).max())
    print(f"{name} {mode}: max|oracle - longdouble| {d:.2e} = {d / spread if spread else np.inf:.1f} spreads (tol {tol:.2e}), |dx| {np.abs(dx).max():.2e}")
    assert d <= tol
    # float64 restatement of the same text: the restatement itself is not what carries the agreement
    as_double = P.restate_step(p, robust=mode == "huber", dtype=np.float64)[0]
    assert np.abs(as_double - restated).max() <= tol
    chi0, _ = P.gate_chi2_after(p, p["pose_cw"])
    over = (p["huber"] > 0) & (chi0 > p["huber"].astype(np.float64) ** 2)
    assert over.any() or len(chi0) <= 6   # (five or six low-noise edges can all lie below delta^2)
    if mode == "huber" and over.any():   # the kernel matters: without it the step is another one
        assert np.abs(P.restate_step(p, robust=False)[0] - pose).max() > 100 * tol
