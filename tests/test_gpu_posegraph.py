"""svgpu_pose_graph_optimize / svgpu_pose_graph_correct_landmarks on the device (tests/posegraph_problems.py holds the yardstick).

The device's optimised Sim3s are compared with the long double restatement: rotation as max |dR|, translation relative to
max(1, |t|), scale relative.  The bound of a case is 16 x the deviation of numpy's own fp64 restatement from the long double one on
that case, floored at FLOOR.  The margin is 16 x because the numeric Jacobians (delta 1e-9) alone carry about 1e-7 of relative rounding
noise, which differs between any two implementations.  FLOOR is the relative residual the device's PCG stops at (1e-14,
posegraph_kernels.h) times the largest condition number of a damped system met on the planted classes (4.4e8, class e, measured with
numpy's eigvalsh on the fp64 form), rounded up: a solve that stops at that residual may be that far from the exact solution.
The final chi2 is held to the same relative bound.
LM iterations, damping trials and stopped-by-gain have to equal the restatement's exactly: the decision filter of
tests/test_posegraph_problem_classes.py makes that a fair demand.  The tests print the figures per case; DESIGN.md section 14."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from tests import posegraph_problems as T

pytestmark = pytest.mark.gpu
FLOOR = 5e-6
SVGPU_ERR_INVALID = 1
ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


def _run(ctx, p, **kw):
    from stella_vslam_amd import optimize
    kw.setdefault("max_iterations", p["max_iter"])
    return optimize.pose_graph_optimize(ctx, p["sim3"], p["fixed"], p["e1"], p["e2"], p["meas"], fix_scale=p["fix_scale"], **kw)


def _bound(case):
    return max(16.0 * T.deviation(T.solved(case, "fp64")["sim3"], T.solved(case, "ld")["sim3"]), FLOOR)


@pytest.mark.parametrize("case", T.CASES)
def test_device_agrees_with_the_long_double_restatement(ctx, case):
    p = T.problem(case)
    ref, f64 = T.solved(case, "ld"), T.solved(case, "fp64")
    out = _run(ctx, p)
    bound = _bound(case)
    dev = T.deviation(out["sim3"], ref["sim3"])
    dchi = abs(out["final_chi2"] - ref["final_chi2"]) / max(abs(ref["final_chi2"]), 1e-300) if ref["final_chi2"] != 0 else abs(out["final_chi2"])
    dpose = float(np.abs(out["pose_cw"].reshape(-1, 12) - np.asarray(ref["pose"], np.float64)).max() / max(1.0, float(np.abs(ref["pose"]).max())))
    print(f"{case}: numpy fp64 {T.deviation(f64['sim3'], ref['sim3']):.2e} bound {bound:.2e} device {dev:.2e} chi2 {dchi:.2e} pose {dpose:.2e} | LM "
          f"{out['lm_iterations']} / {ref['lm_iterations']} trials {out['lm_trials']} / {ref['lm_trials']} gain {out['stopped_by_gain']} / "
          f"{ref['stopped_by_gain']} PCG {out['pcg_iterations']} capped {out['pcg_capped']} free {out['num_free']}")
    assert (out["lm_iterations"], out["lm_trials"], out["stopped_by_gain"]) == (ref["lm_iterations"], ref["lm_trials"], ref["stopped_by_gain"])
    assert dev <= bound
    assert dchi <= bound
    assert dpose <= bound + 2.0 ** -24  # the scale goes through a float before the division
    assert abs(out["initial_chi2"] - ref["initial_chi2"]) <= 1e-9 * max(ref["initial_chi2"], 1e-300) or ref["initial_chi2"] == out["initial_chi2"]
    # fixed vertices, and under fix_scale every scale, come back bit-equal to the input
    fx = p["fixed"].astype(bool)
    assert np.array_equal(out["sim3"][fx].view(np.uint64), p["sim3"][fx].view(np.uint64))
    if p["fix_scale"]:
        assert np.array_equal(out["sim3"][:, 7].view(np.uint64), p["sim3"][:, 7].view(np.uint64))


@pytest.mark.parametrize("case", ["c-fs0", "d65-fs1", "f-fs0"])
def test_two_calls_are_bit_equal(ctx, case):
    p = T.problem(case)
    a, b = _run(ctx, p), _run(ctx, p)
    assert np.array_equal(a["sim3"].view(np.uint64), b["sim3"].view(np.uint64))
    assert np.array_equal(a["pose_cw"].view(np.uint64), b["pose_cw"].view(np.uint64))
    assert (a["lm_iterations"], a["lm_trials"], a["pcg_iterations"], a["final_chi2"]) == (b["lm_iterations"], b["lm_trials"], b["pcg_iterations"], b["final_chi2"])


@pytest.mark.parametrize("case", ["c-fs0", "d63-fs1"])
def test_a_disconnected_neighbour_at_its_minimum_changes_nothing(ctx, case):
    """The problem is optimised alone and with class (h) appended as a second, disconnected component.  The components are coupled
    only through what the LM loop shares: chi2, dx^T (lambda dx + b) and lambda0 = 1e-5 max diag H.  Class (h) is EXACTLY at its
    minimum (identity rotations, integer translations: every error is zero bit for bit), so it adds exact zeros to chi2 and to the
    right-hand side, its dx stays zero, and its translations are small next to the problem's, so the largest diagonal entry of H is the
    problem's own.  The decisions are then the same and the problem's vertices have to agree within the class bound (they are not
    promised bit-equal: the position of a term in a fixed-order sum moves with the numbering)."""
    p, h = T.problem(case), T.problem("h-fs" + case[-1])
    n = len(p["sim3"])
    both = dict(sim3=np.concatenate([p["sim3"], h["sim3"]]), fixed=np.concatenate([p["fixed"], h["fixed"]]), e1=np.concatenate([p["e1"], h["e1"] + n]),
                e2=np.concatenate([p["e2"], h["e2"] + n]), meas=np.concatenate([p["meas"], h["meas"]]), fix_scale=p["fix_scale"], max_iter=p["max_iter"])
    alone, emb = _run(ctx, p), _run(ctx, both)
    assert (alone["lm_iterations"], alone["lm_trials"], alone["stopped_by_gain"]) == (emb["lm_iterations"], emb["lm_trials"], emb["stopped_by_gain"])
    dev = T.deviation(emb["sim3"][:n], alone["sim3"])
    print(f"{case} beside h: {dev:.2e}")
    assert dev <= _bound(case)
    assert np.array_equal(emb["sim3"][n:].view(np.uint64), h["sim3"].view(np.uint64))  # the neighbour did not move


@pytest.mark.parametrize("num", [1, 63, 64, 65, 1000])
def test_landmark_correction_against_numpy(ctx, num):
    from stella_vslam_amd import optimize
    rng = np.random.default_rng(num)
    p = T.problem("c-fs0")
    before, after = p["sim3"], np.asarray(T.solved("c-fs0", "fp64")["sim3"], np.float64)
    ref = rng.integers(0, len(before), size=num).astype(np.int32)
    ref[0] = 0  # vertex 0 is fixed
    pos = rng.normal(size=(num, 3)) * 10.0
    out = optimize.correct_landmarks(ctx, before, after, ref, pos)
    exp = T.correct_landmarks(before.astype(np.longdouble), after.astype(np.longdouble), ref, pos.astype(np.longdouble))
    err = float((np.abs(out - exp).max(1) / np.maximum(1.0, np.abs(exp).max(1))).max())
    print(f"{num} landmarks: {err:.2e}")
    assert err <= 1e-12
    held = ref == 0  # a landmark of a fixed vertex comes back unchanged within rounding
    assert float(np.abs(out[held] - pos[held]).max()) <= 1e-12 * max(1.0, float(np.abs(pos[held]).max()))


def test_iteration_limit(ctx):
    """max_iterations ends the run: two iterations of class c, the same decisions and the same poses as the restatement stopped there."""
    p = T.problem("c-fs0")
    ref, f64 = T.optimize(p, np.longdouble, max_iter=2), T.optimize(p, np.float64, max_iter=2)
    out = _run(ctx, p, max_iterations=2)
    assert (out["lm_iterations"], out["lm_trials"], out["stopped_by_gain"]) == (2, ref["lm_trials"], 0) == (ref["lm_iterations"], ref["lm_trials"], ref["stopped_by_gain"])
    assert T.deviation(out["sim3"], ref["sim3"]) <= max(16.0 * T.deviation(f64["sim3"], ref["sim3"]), FLOOR)
    zero = _run(ctx, p, max_iterations=0)  # nothing but the chi2 of the input
    assert (zero["lm_iterations"], zero["lm_trials"]) == (0, 0) and zero["initial_chi2"] == zero["final_chi2"] > 0
    assert np.array_equal(zero["sim3"].view(np.uint64), p["sim3"].view(np.uint64))


def _launches(L, ctx):
    """launch scopes the k_pg_* profiling classes recorded since svgpu_profile_select("*")"""
    total = 0
    for name in ("k_pg_linearize", "k_pg_assemble", "k_pg_solve", "k_pg_trial", "k_pg_correct_landmarks"):
        ms, n = C.c_double(0), C.c_longlong(0)
        L.svgpu_profile_read_class(ctx.handle, name.encode(), C.byref(ms), C.byref(n))
        total += n.value
    return total


def _bad_inputs():
    p = T.problem("c-fs0")
    base = dict(sim3=p["sim3"], fixed=p["fixed"], e1=p["e1"], e2=p["e2"], meas=p["meas"])

    def mod(**kw):
        d = {k: v.copy() for k, v in base.items()}
        for k, (idx, val) in kw.items():
            d[k][idx] = val
        return d
    yield "index past the end", mod(e1=(2, 8))
    yield "negative index", mod(e2=(1, -1))
    yield "self-edge", mod(e1=(3, int(p["e2"][3])))
    q = mod()
    q["sim3"][4, :4] *= 1.01
    yield "non-unit quaternion", q
    yield "zero scale", mod(sim3=((5, 7), 0.0))
    yield "negative measurement scale", mod(meas=((0, 7), -1.0))
    yield "NaN in a vertex", mod(sim3=((2, 5), np.nan))
    q = mod()
    q["meas"][3, :4] *= 0.99
    yield "non-unit measurement quaternion", q
    yield "no fixed vertex", mod(fixed=(0, 0))
    q = mod()
    q["sim3"] = np.concatenate([q["sim3"], q["sim3"][:1]])
    q["fixed"] = np.concatenate([q["fixed"], [0]]).astype(np.uint8)
    yield "free vertex without an edge", q


@pytest.mark.parametrize("name,bad", list(_bad_inputs()), ids=[n for n, _ in _bad_inputs()])
def test_invalid_input_is_refused_before_any_launch(ctx, name, bad):
    from stella_vslam_amd import optimize
    from stella_vslam_amd._lib import SvgpuError
    from stella_vslam_amd._lib import lib
    L = lib()
    L.svgpu_profile_select(ctx.handle, b"*")
    try:
        with pytest.raises(SvgpuError) as e:
            optimize.pose_graph_optimize(ctx, bad["sim3"], bad["fixed"], bad["e1"], bad["e2"], bad["meas"])
        assert e.value.status == SVGPU_ERR_INVALID
        assert _launches(L, ctx) == 0
    finally:
        L.svgpu_profile_select(ctx.handle, None)


def test_empty_graphs_and_bad_landmark_references_are_refused(ctx):
    from stella_vslam_amd import optimize
    from stella_vslam_amd._lib import SvgpuError
    p = T.problem("a-fs0")
    for kw in (dict(sim3=np.zeros((0, 8)), fixed=np.zeros(0, np.uint8), e1=p["e1"], e2=p["e2"], meas=p["meas"]),
               dict(sim3=p["sim3"], fixed=p["fixed"], e1=np.zeros(0, np.int32), e2=np.zeros(0, np.int32), meas=np.zeros((0, 8)))):
        with pytest.raises(SvgpuError) as e:
            optimize.pose_graph_optimize(ctx, kw["sim3"], kw["fixed"], kw["e1"], kw["e2"], kw["meas"])
        assert e.value.status == SVGPU_ERR_INVALID
    with pytest.raises(SvgpuError) as e:
        optimize.pose_graph_optimize(ctx, p["sim3"], p["fixed"], p["e1"], p["e2"], p["meas"], max_iterations=-1)
    assert e.value.status == SVGPU_ERR_INVALID
    with pytest.raises(SvgpuError) as e:
        optimize.correct_landmarks(ctx, p["sim3"], p["sim3"], np.array([2], np.int32), np.zeros((1, 3)))
    assert e.value.status == SVGPU_ERR_INVALID
    bad = p["sim3"].copy()
    bad[1, 7] = 0.0
    with pytest.raises(SvgpuError) as e:
        optimize.correct_landmarks(ctx, p["sim3"], bad, np.array([0], np.int32), np.zeros((1, 3)))
    assert e.value.status == SVGPU_ERR_INVALID


def test_profiling_classes_are_registered():
    from stella_vslam_amd._lib import lib
    L = lib()
    names = L.svgpu_profile_kernels().decode().split(",")
    assert {"k_pg_linearize", "k_pg_assemble", "k_pg_solve", "k_pg_trial", "k_pg_correct_landmarks"} <= set(names)


# ------------------------------------------------------------------------------------------------ drop-in class
def _stand_in_map():
    """12 keyframes on a circle, chain parents, root = loop keyframe 0, current keyframe 11, keyframes 9 .. 11 pre-corrected, loop
    connections from 10 and 11 to 0 and 1, 40 landmarks with two observations each, two entries in found_lm_to_ref_keyfrm_id."""
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


def test_drop_in_class_equals_the_flat_call_on_the_transcribed_edges(ctx, tmp_path):
    """optimize::hip::graph_optimizer (host/test_graph_optimizer on a map file) against the flat Python calls on the edge list the Python
    transcription of the four loops builds.  Not bit for bit: the class takes the loop connections in pointer order and both sides round
    the Sim3 of a pose on their own, and any last-bit difference of an input is amplified by the numeric Jacobians like the difference
    between two implementations -- so the bound is the floor of the other tests.  The decisions have to be equal."""
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
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    got_pose = np.array([ln[2:] for ln in lines if ln[0] == "KF"], np.float64)
    got_lm = np.array([ln[2:] for ln in lines if ln[0] == "LM"], np.float64)
    got_stats = [int(v) for v in [ln for ln in lines if ln[0] == "STATS"][0][1:]]
    # the flat calls: Sim3s_cw of step 2, the transcription's edges, fixed = root / loop (0) and current (11)
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
    assert (11, 0) in [(a, b) for a, b, _ in edges] and len(edges) > 12
    fixed = np.zeros(len(kfs), np.uint8)
    fixed[[0, 11]] = 1
    flat = optimize.pose_graph_optimize(ctx, sim3_cw, fixed, [a for a, _, _ in edges], [b for _, b, _ in edges], np.array([m for _, _, m in edges]))
    ref = np.array([found.get(l["id"], l["ref"]) for l in lms], np.int32)
    exp_lm = optimize.correct_landmarks(ctx, sim3_cw, flat["sim3"], ref, np.array([l["pos"] for l in lms]))
    dp = float(np.abs(got_pose - flat["pose_cw"].reshape(-1, 12)).max() / max(1.0, float(np.abs(flat["pose_cw"]).max())))
    dl = float(np.abs(got_lm - exp_lm).max() / max(1.0, float(np.abs(exp_lm).max())))
    print(f"drop-in: poses {dp:.2e} landmarks {dl:.2e} LM {got_stats} / {flat['lm_iterations']} {flat['lm_trials']} {flat['stopped_by_gain']} edges {len(edges)}")
    assert got_stats == [flat["lm_iterations"], flat["lm_trials"], flat["stopped_by_gain"]]
    assert dp <= FLOOR + 2.0 ** -24 and dl <= FLOOR + 2.0 ** -24
    assert float(np.abs(exp_lm - np.array([l["pos"] for l in lms])).max()) > 1e-3  # the correction moved something


def test_host_program_of_the_drop_in_class():
    exe = ROOT / "stella_vslam_amd" / "host" / "test_graph_optimizer"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "graph_optimizer ok" in out.stdout
