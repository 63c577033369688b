"""The pose graph's direct solver on the device: svgpu_pose_graph_optimize_ex with the block envelope Cholesky and the solver's self-test
(tests/posegraph_problems.py and tests/posegraph_direct_problems.py hold the yardsticks).

The bound is the one tests/test_gpu_posegraph.py uses, restated here: the device's Sim3s, poses and final chi2 may deviate from the long
double restatement by 16 x the deviation of numpy's own fp64 restatement from it on that case (the numeric Jacobians, delta 1e-9, carry
about 1e-7 of relative rounding noise that differs between any two implementations), floored at 5e-6 (the floor of the PCG's stopping
residual times the largest condition number met; a direct solve needs less, which the printed figures show -- the floor is not tightened
here).  LM iterations, damping trials and stopped-by-gain have to equal the restatement's exactly: the decision filters of the CPU tests
make that a fair demand.  The tests print the figures per case; DESIGN.md section 14."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from tests import posegraph_direct_problems as D
from tests import posegraph_envelope_graphs as G
from tests import posegraph_problems as T

pytestmark = pytest.mark.gpu
FLOOR = 5e-6
SVGPU_ERR_INVALID, SVGPU_ERR_NUMERIC = 1, 6
ROOT = pathlib.Path(__file__).resolve().parent.parent
STATS = ("lm_iterations", "lm_trials", "pcg_iterations", "pcg_capped", "stopped_by_gain", "num_free", "initial_chi2", "final_chi2", "lambda_final")


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


def _run(ctx, p, **kw):
    from stella_vslam_amd import optimize
    kw.setdefault("max_iterations", p["max_iter"])
    return optimize.pose_graph_optimize(ctx, p["sim3"], p["fixed"], p["e1"], p["e2"], p["meas"], fix_scale=p["fix_scale"], **kw)


def _source(case):
    return D if case in D.CASES else T


def _bound(case):
    S = _source(case)
    return max(16.0 * T.deviation(S.solved(case, "fp64")["sim3"], S.solved(case, "ld")["sim3"]), FLOOR)


def _agrees_with_the_long_double_restatement(ctx, case, solver):
    S = _source(case)
    p, ref, f64 = S.problem(case), S.solved(case, "ld"), S.solved(case, "fp64")
    out = _run(ctx, p, solver=solver)
    bound = _bound(case)
    dev = T.deviation(out["sim3"], ref["sim3"])
    dchi = abs(out["final_chi2"] - ref["final_chi2"]) / max(abs(ref["final_chi2"]), 1e-300) if ref["final_chi2"] != 0 else abs(out["final_chi2"])
    dpose = float(np.abs(out["pose_cw"].reshape(-1, 12) - np.asarray(ref["pose"], np.float64)).max() / max(1.0, float(np.abs(ref["pose"]).max())))
    print(f"{case} {solver}: numpy fp64 {T.deviation(f64['sim3'], ref['sim3']):.2e} bound {bound:.2e} device {dev:.2e} chi2 {dchi:.2e} pose {dpose:.2e} | LM "
          f"{out['lm_iterations']} / {ref['lm_iterations']} trials {out['lm_trials']} / {ref['lm_trials']} gain {out['stopped_by_gain']} / "
          f"{ref['stopped_by_gain']} PCG {out['pcg_iterations']} ordering {out['ordering']} blocks {out['envelope_blocks']} tallest column "
          f"{out['max_column_rows']} failed {out['failed_solves']} free {out['num_free']}")
    assert (out["lm_iterations"], out["lm_trials"], out["stopped_by_gain"]) == (ref["lm_iterations"], ref["lm_trials"], ref["stopped_by_gain"])
    assert dev <= bound
    assert dchi <= bound
    assert dpose <= bound + 2.0 ** -24  # the scale goes through a float before the division
    fx = p["fixed"].astype(bool)
    assert np.array_equal(out["sim3"][fx].view(np.uint64), p["sim3"][fx].view(np.uint64))
    if p["fix_scale"]:
        assert np.array_equal(out["sim3"][:, 7].view(np.uint64), p["sim3"][:, 7].view(np.uint64))
    if solver == "envelope":
        nfree, edges = G.from_problem(p)
        assert out["solver"] == 1 and out["pcg_iterations"] == 0 and out["pcg_capped"] == 0 and out["failed_solves"] == 0
        assert out["envelope_blocks"] >= nfree
        if any(a >= 0 and b >= 0 for a, b in edges):
            assert out["envelope_blocks"] > nfree > 0
    else:
        assert out["solver"] == 0 and out["envelope_blocks"] == 0


# ------------------------------------------------------------------------------------------------ 1. parity on the existing classes
@pytest.mark.parametrize("case", T.CASES)
def test_envelope_solver_agrees_with_the_long_double_restatement(ctx, case):
    _agrees_with_the_long_double_restatement(ctx, case, "envelope")


# ------------------------------------------------------------------------------------------------ 2. the new classes, both solvers
@pytest.mark.parametrize("solver", ["pcg", "envelope"])
@pytest.mark.parametrize("case", D.CASES)
def test_new_classes_agree_with_the_long_double_restatement(ctx, case, solver):
    _agrees_with_the_long_double_restatement(ctx, case, solver)


# ------------------------------------------------------------------------------------------------ 3. the PCG path is what it was
class _Options(C.Structure):
    _fields_ = [("solver", C.c_int32), ("reserved", C.c_int32 * 3)]


def _ex(ctx, p, options, want_solver_stats=True):
    """svgpu_pose_graph_optimize_ex called directly (options: None or an _Options)"""
    from stella_vslam_amd import optimize
    from stella_vslam_amd._lib import lib
    s, f, m = np.ascontiguousarray(p["sim3"]), np.ascontiguousarray(p["fixed"]), np.ascontiguousarray(p["meas"])
    e1, e2 = np.ascontiguousarray(p["e1"]), np.ascontiguousarray(p["e2"])
    out, pose, st, sst = np.zeros_like(s), np.zeros((len(s), 3, 4)), optimize._PoseGraphStats(), optimize._PoseGraphSolverStats()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib().svgpu_pose_graph_optimize_ex(ctx.handle, len(s), vp(s), vp(f), len(e1), vp(e1), vp(e2), vp(m), int(p["fix_scale"]), int(p["max_iter"]), 1e-3, vp(out),
                                            vp(pose), C.cast(C.pointer(st), C.c_void_p), None if options is None else C.cast(C.pointer(options), C.c_void_p),
                                            C.cast(C.pointer(sst), C.c_void_p) if want_solver_stats else None)
    res = {k: getattr(st, k) for k in STATS}
    res.update(sim3=out, pose_cw=pose, status=rc)
    return res


@pytest.mark.parametrize("case", ["c-fs0", "d65-fs1", "f-fs0"])
def test_ex_with_pcg_and_with_null_options_is_the_plain_call_bit_for_bit(ctx, case):
    p = T.problem(case)
    plain = _run(ctx, p)
    for other in (_ex(ctx, p, _Options(0, (C.c_int32 * 3)(0, 0, 0))), _ex(ctx, p, None), _ex(ctx, p, None, want_solver_stats=False)):
        assert other["status"] == 0
        assert np.array_equal(plain["sim3"].view(np.uint64), other["sim3"].view(np.uint64))
        assert np.array_equal(plain["pose_cw"].view(np.uint64), other["pose_cw"].view(np.uint64))
        for k in STATS:
            assert np.float64(plain[k]).view(np.uint64) == np.float64(other[k]).view(np.uint64), k
    assert plain["pcg_iterations"] > 0


# ------------------------------------------------------------------------------------------------ 4. repeatability, the neighbour
@pytest.mark.parametrize("case", ["c-fs0", "d65-fs1", "m-fs0"])
def test_two_envelope_calls_are_bit_equal(ctx, case):
    p = _source(case).problem(case)
    a, b = _run(ctx, p, solver="envelope"), _run(ctx, p, solver="envelope")
    assert np.array_equal(a["sim3"].view(np.uint64), b["sim3"].view(np.uint64))
    assert np.array_equal(a["pose_cw"].view(np.uint64), b["pose_cw"].view(np.uint64))
    assert (a["lm_iterations"], a["lm_trials"], a["final_chi2"], a["lambda_final"]) == (b["lm_iterations"], b["lm_trials"], b["final_chi2"], b["lambda_final"])


@pytest.mark.parametrize("case", ["c-fs0", "d63-fs1"])
def test_a_disconnected_neighbour_at_its_minimum_changes_nothing(ctx, case):
    """As in tests/test_gpu_posegraph.py, with the envelope solver: class (h), EXACTLY at its minimum, appended as a second component
    adds exact zeros to chi2 and to the right-hand side and its dx stays zero; the decisions are the same and the problem's vertices
    agree within the class bound (the elimination order, and with it the order of the sums, may change with the numbering)."""
    p, h = T.problem(case), T.problem("h-fs" + case[-1])
    n = len(p["sim3"])
    both = dict(sim3=np.concatenate([p["sim3"], h["sim3"]]), fixed=np.concatenate([p["fixed"], h["fixed"]]), e1=np.concatenate([p["e1"], h["e1"] + n]),
                e2=np.concatenate([p["e2"], h["e2"] + n]), meas=np.concatenate([p["meas"], h["meas"]]), fix_scale=p["fix_scale"], max_iter=p["max_iter"])
    alone, emb = _run(ctx, p, solver="envelope"), _run(ctx, both, solver="envelope")
    assert (alone["lm_iterations"], alone["lm_trials"], alone["stopped_by_gain"]) == (emb["lm_iterations"], emb["lm_trials"], emb["stopped_by_gain"])
    dev = T.deviation(emb["sim3"][:n], alone["sim3"])
    print(f"{case} beside h, envelope: {dev:.2e}")
    assert dev <= _bound(case)
    assert np.array_equal(emb["sim3"][n:].view(np.uint64), h["sim3"].view(np.uint64))  # the neighbour did not move


# ------------------------------------------------------------------------------------------------ 5. the self-test
SELFTEST_GRAPHS = {f"chain of {n}": (lambda n=n: G.chain(n, 3)) for n in (1, 2, 63, 64, 65, 257, 2049)}
SELFTEST_GRAPHS["hub of 40"] = lambda: G.hub(40)
SELFTEST_GRAPHS["every pair of 70"] = lambda: G.dense(70)   # columns taller than a wavefront, and than the LDS staging of a column


@pytest.mark.parametrize("name", list(SELFTEST_GRAPHS))
def test_selftest_solves_diagonally_dominant_systems(ctx, name):
    from stella_vslam_amd import optimize
    nfree, edges = SELFTEST_GRAPHS[name]()
    pa, pb, diag, blocks, rhs = G.system(nfree, edges)
    status, x, st = optimize.envelope_selftest_solve(ctx, pa, pb, diag, blocks, rhs)
    assert status == 0
    res = G.residual(pa, pb, diag, blocks, rhs, x)
    rc, out, info = G.run_check(nfree, edges)
    print(f"{name}: residual {res:.2e} blocks {st['envelope_blocks']} tallest column {st['max_column_rows']} ordering {st['ordering']} | host {info}")
    assert rc == 0, out
    assert res <= 1e-12
    assert (st["envelope_blocks"], st["max_column_rows"], st["ordering"]) == (info["blocks"], info["max_column_rows"], info["ordering"])
    assert st["solver"] == 1 and st["failed_solves"] == 0


def test_selftest_reports_an_indefinite_system(ctx):
    from stella_vslam_amd import optimize
    nfree, edges = G.chain(65, 3)
    pa, pb, diag, blocks, rhs = G.system(nfree, edges)
    diag[nfree // 2] *= -1.0
    status, x, st = optimize.envelope_selftest_solve(ctx, pa, pb, diag, blocks, rhs)
    assert status == SVGPU_ERR_NUMERIC and st["failed_solves"] == 1
    assert not x.any()  # the output is untouched


# ------------------------------------------------------------------------------------------------ 6. error paths
PG_CLASSES = ("k_pg_linearize", "k_pg_assemble", "k_pg_solve", "k_pg_trial", "k_pg_correct_landmarks", "k_pg_env_assemble", "k_pg_env_factor_solve")


def _launches(L, ctx):
    """launch scopes the k_pg_* profiling classes recorded since svgpu_profile_select("*")"""
    total = 0
    for name in PG_CLASSES:
        ms, n = C.c_double(0), C.c_longlong(0)
        L.svgpu_profile_read_class(ctx.handle, name.encode(), C.byref(ms), C.byref(n))
        total += n.value
    return total


@pytest.mark.parametrize("options", [(2, (0, 0, 0)), (-1, (0, 0, 0)), (1, (0, 1, 0)), (0, (0, 0, 7))], ids=["solver 2", "solver -1", "reserved[1]", "reserved[2] with pcg"])
def test_bad_options_are_refused_before_any_launch(ctx, options):
    from stella_vslam_amd._lib import lib
    L = lib()
    p = T.problem("c-fs0")
    L.svgpu_profile_select(ctx.handle, b"*")
    try:
        out = _ex(ctx, p, _Options(options[0], (C.c_int32 * 3)(*options[1])))
        assert out["status"] == SVGPU_ERR_INVALID
        assert _launches(L, ctx) == 0
        assert not out["sim3"].any()
        good = _ex(ctx, p, _Options(1, (C.c_int32 * 3)(0, 0, 0)))  # the counter does count: a good call records launches
        assert good["status"] == 0 and _launches(L, ctx) > 0
    finally:
        L.svgpu_profile_select(ctx.handle, None)


def test_profiling_classes_are_registered():
    from stella_vslam_amd._lib import lib
    L = lib()
    assert set(PG_CLASSES) <= set(L.svgpu_profile_kernels().decode().split(","))


# ------------------------------------------------------------------------------------------------ 7. drop-in class
def _stand_in_map():
    """The map tests/test_gpu_posegraph.py hands to the host program: 12 keyframes on a circle, chain parents, root = loop keyframe 0,
    current keyframe 11, keyframes 9 .. 11 pre-corrected, loop connections from 10 and 11 to 0 and 1, 40 landmarks."""
    rng = np.random.default_rng(12)
    n = 12
    S = T._trajectory(rng, n, radius=4.0)
    corr = T.make_sim3(np.array([0.02, -0.03, 0.01]), np.array([0.2, -0.1, 0.15]), 1.05)
    kfs = []
    for k in range(n):
        cov = [(j, 200 - 30 * abs(j - k)) for j in range(n) if j != k and abs(j - k) <= 3]
        if k >= 10:
            cov += [(k - 10, 105), (k - 9, 60)]
        if k <= 1:
            cov += [(k + 10, 105)]
        if 1 <= k <= 2:
            cov += [(k + 9, 60)]
        cov.sort(key=lambda c: (-c[1], -c[0]))
        pre = k >= 9
        kfs.append(dict(id=k, erased=0, parent=k - 1, loop=[], covis=cov, pose=T.sim3_to_pose(S[k]), non=S[k] if pre else None,
                        pre=T.sim3_mul(corr, S[k]) if pre else None))
    conns = [(11, [0, 1]), (10, [0, 1])]
    lms = []
    for l in range(40):
        ref = l % n
        pc = np.array([0.3 * np.sin(1.0 + l), 0.2 * np.cos(2.0 * l), 3.0 + 0.1 * (l % 7)])
        lms.append(dict(id=l, ref=ref, pos=T.sim3_map(T.sim3_inv(S[ref]), pc), obs=[ref, (ref + 1) % n]))
    return kfs, conns, lms, {3: 11, 5: 0}


def test_drop_in_class_with_the_envelope_solver_equals_the_flat_call(ctx, tmp_path):
    from stella_vslam_amd import optimize
    exe = ROOT / "stella_vslam_amd" / "host" / "test_graph_optimizer"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    kfs, conns, lms, found = _stand_in_map()
    f = lambda v: " ".join(repr(float(x)) for x in v)
    out = [f"{len(kfs)} 11 0 100 0"]
    for k in kfs:
        zero = np.zeros(8)
        out.append(f"{k['id']} {k['parent']} {int(k['parent'] < 0)} 0 {f(k['pose'])} {int(k['non'] is not None)} {f(k['non'] if k['non'] is not None else zero)} "
                   f"{int(k['pre'] is not None)} {f(k['pre'] if k['pre'] is not None else zero)} 0 {len(k['covis'])} " + " ".join(f"{i} {w}" for i, w in k["covis"]))
    out.append(str(len(conns)))
    out += [f"{i} {len(ids)} " + " ".join(map(str, ids)) for i, ids in conns]
    out.append(str(len(lms)))
    out += [f"{l['id']} {l['ref']} {f(l['pos'])} {len(l['obs'])} " + " ".join(map(str, l["obs"])) for l in lms]
    out.append(str(len(found)))
    out += [f"{a} {b}" for a, b in found.items()]
    path = tmp_path / "map.txt"
    path.write_text("\n".join(out) + "\n")
    r = subprocess.run([str(exe), str(path), "envelope"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    got_pose = np.array([ln[2:] for ln in lines if ln[0] == "KF"], np.float64)
    got_stats = [int(v) for v in [ln for ln in lines if ln[0] == "STATS"][0][1:]]
    sim3_cw = []
    for k in kfs:
        if k["pre"] is not None:
            sim3_cw.append(k["pre"])
        else:
            P = k["pose"].reshape(3, 4)
            q = T.rot_to_quat(P[:, :3])
            sim3_cw.append(np.concatenate([q / np.sqrt((q * q).sum()), P[:, 3], [1.0]]))
    sim3_cw = np.array(sim3_cw)
    edges = T.transcribe_edges([dict(k, cw=sim3_cw[i]) for i, k in enumerate(kfs)], conns, 11, 0, 100)
    fixed = np.zeros(len(kfs), np.uint8)
    fixed[[0, 11]] = 1
    flat = optimize.pose_graph_optimize(ctx, sim3_cw, fixed, [a for a, _, _ in edges], [b for _, b, _ in edges], np.array([m for _, _, m in edges]), solver="envelope")
    dp = float(np.abs(got_pose - flat["pose_cw"].reshape(-1, 12)).max() / max(1.0, float(np.abs(flat["pose_cw"]).max())))
    print(f"drop-in, envelope: poses {dp:.2e} LM {got_stats} / {flat['lm_iterations']} {flat['lm_trials']} {flat['stopped_by_gain']} edges {len(edges)}")
    assert got_stats[:3] == [flat["lm_iterations"], flat["lm_trials"], flat["stopped_by_gain"]]
    assert got_stats[3:] == [1, flat["envelope_blocks"]]   # the envelope solver did run in the class
    assert dp <= FLOOR + 2.0 ** -24


def test_host_program_of_the_drop_in_class_with_the_envelope_solver():
    exe = ROOT / "stella_vslam_amd" / "host" / "test_graph_optimizer"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe), "envelope"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "graph_optimizer ok" in out.stdout
