"""GPU parity of ONE damped bundle-adjustment step, per reduced-system solver, at the size boundaries of those solvers
(tests/ba_step_problems.py; the classes are held to their claims on the CPU by tests/test_ba_step_problem_classes.py).

After one accepted trial the output is x0 [+] dx: nothing corrects an error of the Schur complement, the right-hand side, the
factorisation or the back-substitution.  Poses and points are held entry-wise to the CPU oracle within
    tol = max(1024 * spread, 64 ulp of the largest pose entry)
where `spread` is the oracle's own reorder noise on that problem (max|delta| between the scene and its reversed-observation copy,
recomputed here).  The device sums the same terms in other groupings and eliminates in another order; both scale with the same
cond * eps as the reorder spread, which the factor 1024 absorbs.  The bound is taken against the oracle, never against another solver.
The PCG forms (and AUTO, which resolves to one at F = 85) run with pcg_tolerance = 1e-14, so the same bound applies to them.

No PCG stagnated above that: no class is loosened.

Measured on an MI355X, max|delta| / spread as "poses / points" per (problem, solver); the bound is 1024, the largest is 5.8 (tiny_f1, pcg):
problem                               auto       cholesky  cholesky_mfma            pcg      pcg_multi          dense       envelope
tiny_f1                          4.5 / 5.5      4.5 / 5.5      4.5 / 5.5      4.5 / 5.8      4.5 / 5.8      4.5 / 5.2      4.5 / 5.2
tiny_f2                          2.1 / 2.9      2.1 / 2.9      2.1 / 2.8      2.1 / 2.8      2.1 / 3.0      2.1 / 2.8      2.1 / 2.7
tiny_f3                          3.2 / 2.3      3.2 / 2.3      3.2 / 2.6      4.8 / 2.6      4.8 / 2.6      3.2 / 2.4      3.2 / 2.3
panel_f8                         2.9 / 1.9      2.9 / 1.9      2.9 / 1.7      3.0 / 1.6      3.2 / 1.8      2.9 / 1.8      2.8 / 1.6
panel_f16                        0.6 / 0.6      0.6 / 0.6      0.9 / 0.7      0.9 / 0.8      0.9 / 0.8      0.9 / 0.8      0.9 / 0.7
onchip_f21                       1.0 / 1.3      1.0 / 1.3      0.8 / 1.0      0.9 / 1.1      1.0 / 1.1      0.8 / 1.0      0.9 / 1.0
onchip_f22                       1.2 / 1.0      1.2 / 1.0      1.2 / 1.0      1.5 / 1.2      1.4 / 1.1      1.5 / 1.1      1.5 / 1.2
onchip_f23                       1.6 / 1.4              -              -      1.6 / 1.4      1.6 / 1.5      1.6 / 1.4      1.6 / 1.5
dense_f24                        1.9 / 2.1              -              -      1.3 / 1.5      1.3 / 1.5      1.9 / 2.1      1.5 / 1.8
dense_f25                        3.4 / 2.3              -              -      3.5 / 2.4      3.6 / 2.6      3.4 / 2.3      3.1 / 2.3
dense_f32                        1.5 / 1.4              -              -      1.4 / 1.3      1.4 / 1.3      1.5 / 1.4      1.4 / 1.4
dense_f38                        0.6 / 0.5              -              -      0.6 / 0.4      0.6 / 0.4      0.6 / 0.5      0.6 / 0.4
pcg_f85                          1.6 / 3.8              -              -      1.6 / 3.8      1.6 / 3.8      1.2 / 3.2      1.1 / 3.2
pcg_f86                          0.9 / 3.3              -              -      1.9 / 4.0      1.9 / 4.0      0.8 / 3.3      0.9 / 3.3
pattern_blockdiag                2.2 / 2.8      2.2 / 2.8      2.4 / 3.0      2.2 / 2.8      2.2 / 2.8      2.4 / 3.0      2.3 / 2.9
pattern_arrow_hub_first          0.9 / 2.1      0.9 / 2.1      1.0 / 2.1      0.9 / 2.1      0.9 / 2.1      0.8 / 2.1      0.8 / 2.2
pattern_arrow_hub_last           1.2 / 2.8      1.2 / 2.8      1.3 / 2.0      1.2 / 2.5      1.2 / 2.5      1.3 / 2.3      1.3 / 2.7
envelope_one_sided                       -              -              -              -              -              -      0.9 / 2.0
envelope_two_sided                       -              -              -              -              -              -      0.9 / 2.0
envelope_2_cuts                          -              -              -              -              -              -      0.9 / 2.0
envelope_3_cuts                          -              -              -              -              -              -      0.9 / 2.0
envelope_no_band                         -              -              -              -              -              -      0.9 / 2.0
camera_stereo_f22                0.9 / 1.2      0.9 / 1.2      0.9 / 1.2      1.0 / 1.2      0.9 / 1.1      1.1 / 1.2      1.0 / 1.4
camera_equirect_f22              0.9 / 0.6      0.9 / 0.6      0.9 / 0.6      0.8 / 0.7      0.8 / 0.8      0.8 / 0.7      0.9 / 0.8
fixed_points_no_kernel_f22       1.2 / 1.1      1.2 / 1.1      1.2 / 1.1      2.2 / 1.2      2.2 / 1.2      1.1 / 0.9      1.1 / 1.0
("-": the on-chip LL^T does not fit LDS beyond F = 22; the envelope forms are the envelope solver's alone.)
"""
import numpy as np
import pytest

from tests import ba_step_problems as B

pytestmark = pytest.mark.gpu
K_SPREAD = 1024
PCG_TOLERANCE = 1e-14


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd import feature
    return feature.Context()


def _code(solver):
    from stella_vslam_amd import optimize as o
    return dict(auto=o.SOLVER_AUTO, cholesky=o.SOLVER_CHOLESKY, cholesky_mfma=o.SOLVER_CHOLESKY_MFMA, pcg=o.SOLVER_PCG, pcg_multi=o.SOLVER_PCG_MULTI,
                dense=o.SOLVER_DENSE, envelope=o.SOLVER_ENVELOPE)[solver]


def _resolves_to(p, sc, solver):
    """The solver a request ends at (ba_plan.h): the PCG lives in one workgroup's LDS while n <= 512 and the blocks fit -- up to 48 free
    keyframes every upper block is kept, beyond only those that hold a term."""
    if solver == "auto":
        return p["auto"]
    if solver == "pcg":
        F = p["F"]
        NB = F * (F + 1) // 2 if F <= 48 else len(B.kept_upper_blocks(sc))
        fits = p["n"] <= B.PCG_LDS_MAX_UNKNOWNS and B.pcg_lds_bytes(F, NB) <= B.PCG_LDS_MAX_BYTES
        return "pcg_lds" if fits else "pcg_multi"
    return "cholesky" if solver == "cholesky_mfma" else solver


def _run(ctx, p, sc, solver):
    from stella_vslam_amd import optimize
    adj = optimize.local_bundle_adjuster(num_first_iter=1, num_second_iter=0, ctx=ctx).set_solver(_code(solver), pcg_tolerance=PCG_TOLERANCE)
    got = adj.optimize_flat(sc) if p["form"] == "local" else adj.optimize_global_flat(sc, num_iter=1)
    got["resolved"] = adj.last_solver()
    got["plan"] = adj.last_envelope_plan() if got["resolved"] == "envelope" else None
    return got


@pytest.mark.parametrize("name", B.NAMES)
def test_one_step_matches_the_oracle_with_every_solver(ctx, name, monkeypatch):
    p, sc = B.BY_NAME[name], B.scene(name)
    ref, spread_pose, spread_points = B.oracle_reference(name)
    assert 0 < spread_pose < 1e-12 and 0 < spread_points < 1e-12
    floor = 64 * float(np.spacing(np.abs(ref["pose_cw"]).max()))
    tol_pose, tol_points = max(K_SPREAD * spread_pose, floor), max(K_SPREAD * spread_points, floor)
    for k in B.SKY_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in p["env"].items():
        monkeypatch.setenv(k, v)
    runs, failures = {}, []

    def check(ok, what):
        if not ok:
            failures.append(what)

    for solver in p["solvers"]:
        got = runs[solver] = _run(ctx, p, sc, solver)
        gs = got["stats"]
        d_pose, d_points = float(np.abs(got["pose_cw"] - ref["pose_cw"]).max()), float(np.abs(got["points"] - ref["points"]).max())
        print(f"{name:27s} {solver:13s} -> {got['resolved']:9s} max|d| / spread: poses {d_pose / spread_pose:7.1f}  points {d_points / spread_points:7.1f}"
              f"   (|d| {d_pose:.1e} / {d_points:.1e}, tol {tol_pose:.1e} / {tol_points:.1e}, pcg iterations {gs['pcg_iterations']})")
        # the case reached what it was built for
        check(got["rc"] == 0, f"{solver}: rc {got['rc']}")
        check(got["resolved"] == _resolves_to(p, sc, solver), f"{solver}: resolved to {got['resolved']}")
        check((gs["pcg_iterations"] > 0) == (got["resolved"] in ("pcg_lds", "pcg_multi")), f"{solver}: pcg_iterations {gs['pcg_iterations']}")
        check(gs["cholesky_failures"] == 0, f"{solver}: cholesky_failures {gs['cholesky_failures']}")
        if p["plan"]:
            check(got["plan"]["kind"] == p["plan"], f"{solver}: envelope plan {got['plan']}")
            if "SVGPU_SKY_SEGMENTS" in p["env"] and p["plan"] == "segmented":
                check(got["plan"]["cuts"] == int(p["env"]["SVGPU_SKY_SEGMENTS"]) and got["plan"]["jobs"] >= 2, f"{solver}: envelope plan {got['plan']}")
        # the schedule, the sums and the gate
        check(gs["iters_stage1"] == 1 == ref["iters_stage1"] and gs["iters_stage2"] == 0 == ref["iters_stage2"], f"{solver}: schedule {gs}")
        check(gs["chi2_initial"] == pytest.approx(ref["chi2_initial"], rel=1e-12), f"{solver}: chi2_initial {gs['chi2_initial']!r} vs {ref['chi2_initial']!r}")
        check(gs["chi2_final"] == pytest.approx(ref["chi2_final"], rel=1e-9), f"{solver}: chi2_final {gs['chi2_final']!r} vs {ref['chi2_final']!r}")
        if p["form"] == "local":
            check(gs["stage2_entered"] == 1 and gs["num_gated"] == ref["num_gated"], f"{solver}: num_gated {gs['num_gated']} vs {ref['num_gated']}")
            check(np.array_equal(got["outlier"], ref["outlier"]), f"{solver}: outlier flags differ")
        else:
            check(gs["stage2_entered"] == 0 and gs["num_gated"] == 0, f"{solver}: the global form gated")
        # the step itself
        check(d_pose <= tol_pose, f"{solver}: poses off by {d_pose:.3e} = {d_pose / spread_pose:.0f} spreads (tol {tol_pose:.3e})")
        check(d_points <= tol_points, f"{solver}: points off by {d_points:.3e} = {d_points / spread_points:.0f} spreads (tol {tol_points:.3e})")
        if sc.get("point_fixed") is not None:
            fixed = sc["point_fixed"] == 1
            check(np.array_equal(got["points"][fixed], sc["points"][fixed]), f"{solver}: a fixed point moved")
        check(np.array_equal(got["pose_cw"][sc["pose_fixed"] == 1], sc["pose_cw"][sc["pose_fixed"] == 1]), f"{solver}: a fixed pose moved")
        again = _run(ctx, p, sc, solver)  # fixed-order sums
        check(np.array_equal(again["pose_cw"], got["pose_cw"]) and np.array_equal(again["points"], got["points"]), f"{solver}: a second run differs in bits")

    first = runs[p["solvers"][0]]
    for solver, got in runs.items():
        check(got["stats"]["lm_trials"] == first["stats"]["lm_trials"], f"{solver}: lm_trials {got['stats']['lm_trials']} vs {first['stats']['lm_trials']}")
        for other, o in runs.items():
            if other < solver:
                check(np.abs(got["pose_cw"] - o["pose_cw"]).max() <= tol_pose and np.abs(got["points"] - o["points"]).max() <= tol_points,
                      f"{solver} and {other} disagree beyond the tolerance")
    if p["tiled"]:  # AUTO took the tiled dense LL^T: the bits of `dense`, not those of the envelope factorisation
        a, d, e = runs["auto"], runs["dense"], runs["envelope"]
        check(np.array_equal(a["pose_cw"], d["pose_cw"]) and np.array_equal(a["points"], d["points"]), "auto differs in bits from dense")
        check(not np.array_equal(a["pose_cw"], e["pose_cw"]), "auto has the bits of envelope")
    assert not failures, "\n".join(failures)


def test_the_pcg_takes_its_lds_form_below_512_unknowns_and_a_launch_per_iteration_above(ctx):
    """F = 85 (n = 510) against F = 86 (n = 516): svgpu_ba_last_solver tells the two PCG forms apart; both were iterated."""
    forms = {}
    for name in ("pcg_f85", "pcg_f86"):
        got = _run(ctx, B.BY_NAME[name], B.scene(name), "pcg")
        assert got["rc"] == 0 and got["stats"]["pcg_iterations"] > 0
        forms[name] = got["resolved"]
    assert forms == dict(pcg_f85="pcg_lds", pcg_f86="pcg_multi")
