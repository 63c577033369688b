"""svgpu_sim3_transform_optimize / _batch on the device (tests/sim3opt_problems.py holds the yardstick).

Statuses, num_inliers, the early-return flag and the LM iterations and trials per stage have to equal the long double restatement's
exactly: the decision filter of tests/test_sim3opt_problem_classes.py makes that a fair demand, and no case is exempted.  The optimised
Sim3 is compared by deviation() (rotation as max |dR|, translation relative to max(1, |t|), scale relative); the bound of a case is
16 x max(the deviation of numpy's own fp64 restatement from the long double one on that case, F), F being the median of that two-form
deviation over all cases, computed by the module.  The 16 x follows the pose-graph tests: the numeric Jacobians (delta 1e-9) alone carry
about 1e-7 of relative rounding noise that differs between any two implementations; F keeps a case whose two forms agree by luck from
getting a bound below that common noise.  The last robust chi2 of each stage is held to the same relative bound.  The tests print the
figures per case; DESIGN.md section 15."""
import pathlib
import subprocess

import numpy as np
import pytest

from tests import sim3opt_problems as T

pytestmark = pytest.mark.gpu
SVGPU_ERR_INVALID = 1
ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


def _views(p):
    return (p["cam1"], p["pose1"]), (p["cam2"], p["pose2"])


def _run(ctx, p, **kw):
    from stella_vslam_amd import optimize
    v1, v2 = _views(p)
    kw.setdefault("num_iter", p["num_iter"])
    kw.setdefault("fix_scale", p["fix_scale"])
    kw.setdefault("chi_sq", float(p["chi_sq"]))
    return optimize.sim3_transform_optimize(ctx, v1, v2, p["obs1"], p["obs2"], p["w1"], p["w2"], p["pos1"], p["pos2"], p["sim3"], **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


@pytest.mark.parametrize("case", T.CASES)
def test_device_agrees_with_the_long_double_restatement(ctx, case):
    p = T.problem(case)
    ref = T.solved(case, "ld")
    out = _run(ctx, p)
    bound = T.bound(case)
    dev = T.deviation(out["sim3"][None], np.asarray(ref["sim3"])[None])
    dchi = max(_rel(float(out["last_chi2"][s]), ref["last_chi2"][s]) for s in range(2))
    print(f"{case}: numpy fp64 {T.two_form_deviation(case):.2e} bound {bound:.2e} device {dev:.2e} chi2 {dchi:.2e} | iterations {list(out['lm_iterations'])} "
          f"trials {list(out['lm_trials'])} survivors {out['num_survivors']} inliers {out['num_inliers']} early {out['early_return']}")
    assert np.array_equal(out["status"], ref["status"])
    assert (out["num_inliers"], out["early_return"], out["num_survivors"]) == (ref["num_inliers"], ref["early_return"], ref["survivors"])
    assert list(out["lm_iterations"]) == ref["lm_iterations"] and list(out["lm_trials"]) == ref["lm_trials"]
    assert dev <= bound
    assert dchi <= bound
    assert _rel(float(out["first_chi2"][0]), ref["first_chi2"][0]) <= 1e-9
    if p["fix_scale"]:
        assert np.array_equal(_bits(out["sim3"][7:]), _bits(p["sim3"][7:]))
    if ref["early_return"]:
        assert np.array_equal(_bits(out["sim3"]), _bits(p["sim3"]))


def test_an_empty_problem_returns_its_input(ctx):
    p = T.problem("a-fs0")
    q = dict(p, obs1=np.zeros((0, 2)), obs2=np.zeros((0, 2)), w1=np.zeros(0, np.float32), w2=np.zeros(0, np.float32), pos1=np.zeros((0, 3)), pos2=np.zeros((0, 3)))
    out = _run(ctx, q)
    assert (out["num_inliers"], out["early_return"], list(out["lm_iterations"]), list(out["lm_trials"])) == (0, 1, [0, 0], [0, 0])
    assert np.array_equal(_bits(out["sim3"]), _bits(p["sim3"]))


@pytest.mark.parametrize("case", ["b-fs0", "g129-fs1"])
def test_num_iter_zero_keeps_the_survivors_of_stage_one(ctx, case):
    p = T.problem(case)
    ref = T.optimize(p, np.longdouble, num_iter=0)
    out = _run(ctx, p, num_iter=0)
    assert list(out["lm_iterations"]) == [5, 0] and list(out["lm_trials"])[1] == 0
    assert out["num_inliers"] == out["num_survivors"] == ref["survivors"] and not (out["status"] == 2).any()
    assert np.array_equal(out["status"], ref["status"])
    assert T.deviation(out["sim3"][None], np.asarray(ref["sim3"])[None]) <= T.bound(case)


def _same(a, b):
    return (np.array_equal(_bits(a["sim3"]), _bits(b["sim3"])) and np.array_equal(a["status"], b["status"]) and int(a["num_inliers"]) == int(b["num_inliers"])
            and all(np.array_equal(_bits(np.asarray(a[k], np.float64)), _bits(np.asarray(b[k], np.float64))) for k in ("first_chi2", "last_chi2", "lambda_final"))
            and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("lm_iterations", "lm_trials", "early_return", "num_survivors")))


def test_two_calls_and_any_batch_position_are_bit_equal(ctx):
    from stella_vslam_amd import optimize
    pa, pb = T.problem("b-fs0"), T.problem("g128-fs0")
    assert pa["fix_scale"] == pb["fix_scale"]
    one = [_run(ctx, pa), None, _run(ctx, pb)]
    assert _same(one[0], _run(ctx, pa)) and _same(one[2], _run(ctx, pb))
    empty = dict(pa, obs1=np.zeros((0, 2)), obs2=np.zeros((0, 2)), w1=np.zeros(0, np.float32), w2=np.zeros(0, np.float32), pos1=np.zeros((0, 3)), pos2=np.zeros((0, 3)))
    one[1] = _run(ctx, empty)
    probs = [pa, empty, pb]
    for order in ([0, 1, 2], [2, 1, 0]):
        q = [probs[k] for k in order]
        off = np.concatenate([[0], np.cumsum([len(x["obs1"]) for x in q])]).astype(np.int32)
        cat = lambda k, d: np.concatenate([np.asarray(x[k], d).reshape((len(x["obs1"]),) + np.asarray(x[k]).shape[1:]) for x in q])
        out = optimize.sim3_transform_optimize_batch(ctx, [_views(x)[0] for x in q], [_views(x)[1] for x in q], off, cat("obs1", np.float64), cat("obs2", np.float64),
                                                     cat("w1", np.float32), cat("w2", np.float32), cat("pos1", np.float64), cat("pos2", np.float64),
                                                     np.array([x["sim3"] for x in q]), chi_sq=float(pa["chi_sq"]), fix_scale=pa["fix_scale"], num_iter=pa["num_iter"])
        for slot, k in enumerate(order):
            got = dict(sim3=out["sim3"][slot], status=out["status"][off[slot]:off[slot + 1]], num_inliers=out["num_inliers"][slot])
            got.update({f: out[f][slot] for f in ("first_chi2", "last_chi2", "lambda_final", "lm_iterations", "lm_trials", "early_return", "num_survivors")})
            assert _same(got, one[k]), (order, slot)
    # view 1 shared by all problems: the same results again
    q = [pa, pa]
    off = np.array([0, len(pa["obs1"]), 2 * len(pa["obs1"])], np.int32)
    two = lambda k: np.concatenate([pa[k], pa[k]])
    out = optimize.sim3_transform_optimize_batch(ctx, _views(pa)[0], [_views(pa)[1]] * 2, off, two("obs1"), two("obs2"), two("w1"), two("w2"), two("pos1"), two("pos2"),
                                                 np.array([pa["sim3"]] * 2), chi_sq=float(pa["chi_sq"]), fix_scale=pa["fix_scale"], num_iter=pa["num_iter"])
    assert np.array_equal(_bits(out["sim3"][0]), _bits(one[0]["sim3"])) and np.array_equal(_bits(out["sim3"][1]), _bits(one[0]["sim3"]))


def test_an_empty_batch_is_a_success(ctx):
    from stella_vslam_amd import optimize
    out = optimize.sim3_transform_optimize_batch(ctx, [], [], np.zeros(1, np.int32), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros(0, np.float32),
                                                 np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 8)))
    assert len(out["sim3"]) == 0 and len(out["num_inliers"]) == 0


def _bad_calls():
    p = T.problem("a-fs0")

    def mod(**kw):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        for k, (idx, val) in kw.items():
            d[k][idx] = val
        return d
    q = mod()
    q["sim3"][:4] *= 1.0 + 1e-6
    yield "non-unit quaternion", q, {}
    yield "zero scale", mod(sim3=(7, 0.0)), {}
    yield "infinite scale", mod(sim3=(7, np.inf)), {}
    yield "negative inv_sigma_sq", mod(w1=(3, -1.0)), {}
    yield "NaN inv_sigma_sq", mod(w2=(5, np.nan)), {}
    yield "zero chi_sq", mod(), dict(chi_sq=0.0)
    yield "infinite chi_sq", mod(), dict(chi_sq=np.inf)
    yield "negative num_iter", mod(), dict(num_iter=-1)
    q = mod()
    q["cam2"] = dict(q["cam2"], model=7)
    yield "unknown camera model", q, {}


@pytest.mark.parametrize("name,bad,kw", list(_bad_calls()), ids=[n for n, _, _ in _bad_calls()])
def test_invalid_input_is_refused_before_any_launch(ctx, name, bad, kw):
    import ctypes as C
    from stella_vslam_amd._lib import SvgpuError, lib
    L = lib()
    L.svgpu_profile_select(ctx.handle, b"*")
    try:
        with pytest.raises(SvgpuError) as e:
            _run(ctx, bad, **kw)
        assert e.value.status == SVGPU_ERR_INVALID
        ms, n = C.c_double(0), C.c_longlong(0)
        L.svgpu_profile_read_class(ctx.handle, b"k_sim3_opt", C.byref(ms), C.byref(n))
        assert n.value == 0
    finally:
        L.svgpu_profile_select(ctx.handle, None)


def test_null_pointers_offsets_and_untouched_outputs(ctx):
    import ctypes as C
    from stella_vslam_amd import optimize
    from stella_vslam_amd._lib import lib
    L = lib()
    p = T.problem("a-fs0")
    n = len(p["obs1"])
    V1, V2 = optimize._sim3opt_view(*_views(p)[0]), optimize._sim3opt_view(*_views(p)[1])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    arrays = [np.ascontiguousarray(p[k], d) for k, d in (("obs1", np.float64), ("obs2", np.float64), ("w1", np.float32), ("w2", np.float32), ("pos1", np.float64),
                                                        ("pos2", np.float64), ("sim3", np.float64))]
    out, inl, status = np.full(8, 7.5), np.full(1, -3, np.int32), np.full(n, 9, np.uint8)

    def call(off, drop=None, out_ptr=True):
        ptrs = [None if k == drop else vp(a) for k, a in enumerate(arrays)]
        off = np.asarray(off, np.int32)
        return L.svgpu_sim3_transform_optimize_batch(ctx.handle, 1, C.byref(V1), 1, C.byref(V2), vp(off), *ptrs, C.c_float(10.0), 0, 4, vp(out) if out_ptr else None,
                                                     vp(inl), vp(status), None)
    assert call([0, n]) == 0 and out[0] != 7.5  # the well-formed call works with stats == NULL
    out[:], inl[:], status[:] = 7.5, -3, 9
    assert call([0, -1]) == SVGPU_ERR_INVALID          # non-monotone
    assert call([1, n]) == SVGPU_ERR_INVALID           # does not start at 0
    for drop in range(7):
        assert call([0, n], drop=drop) == SVGPU_ERR_INVALID, drop
    assert call([0, n], out_ptr=False) == SVGPU_ERR_INVALID
    assert L.svgpu_sim3_transform_optimize_batch(ctx.handle, 1, None, 1, C.byref(V2), vp(np.array([0, n], np.int32)), *[vp(a) for a in arrays], C.c_float(10.0), 0, 4,
                                                 vp(out), vp(inl), vp(status), None) == SVGPU_ERR_INVALID
    assert (out == 7.5).all() and inl[0] == -3 and (status == 9).all()  # a refused call writes nothing


def test_profiling_class_is_registered():
    import ctypes as C
    from stella_vslam_amd._lib import lib
    L = lib()
    assert "k_sim3_opt" in L.svgpu_profile_kernels().decode().split(",")


# ------------------------------------------------------------------------------------------------ the regime the loop detector runs
@pytest.mark.parametrize("fix_scale", [0, 1])
def test_converged_result_on_a_well_conditioned_scene(ctx, fix_scale):
    """Points 4 .. 9 deep, a quarter gross mismatches, num_iter = 10 as module::loop_detector calls it.  Levenberg-Marquardt is at the
    rounding floor of chi2 long before the last iteration, so which trials are accepted there is rounding noise and the trial sequence is
    NOT compared; the converged Sim3 and the inlier set are.  Bound 1e-6: the minimum is well determined here (the two numpy forms end
    3e-9 .. 1e-8 apart on such scenes), so an arithmetic error of relative size 1e-4 in a projection or in the Sim3 map, which the
    parity bounds of the planted cases would let through, moves the result far beyond it."""
    p = T._scene(7, 60, T.pinhole(), T.pinhole(480.0, 482.0, 330.0, 250.0), bool(fix_scale), 10, gross=15, depth=(4.0, 9.0))
    ref = T.optimize(p, np.longdouble)
    out = _run(ctx, p)
    dev = T.deviation(out["sim3"][None], np.asarray(ref["sim3"])[None])
    print(f"well-conditioned fs{fix_scale}: device {dev:.2e}, inliers {out['num_inliers']} / {ref['num_inliers']}, trials {list(out['lm_trials'])} / {ref['lm_trials']}")
    assert np.array_equal(out["status"], ref["status"]) and out["num_inliers"] == ref["num_inliers"] == 45
    assert list(out["lm_iterations"])[0] == 5
    assert dev <= 1e-6
    assert T.deviation(out["sim3"][None], p["true"][None]) < 5e-3  # and it is the planted transform


# ------------------------------------------------------------------------------------------------ drop-in class
def _orb_inv_level_sigma_sq(levels=8):
    sf = [np.float32(1.0)]
    for _ in range(1, levels):
        sf.append(np.float32(1.2) * sf[-1])
    return np.array([np.float32(1.0) / (s * s) for s in sf], np.float32)


def test_drop_in_class_equals_the_flat_call_on_the_filtered_arrays(ctx, tmp_path):
    """optimize::hip::transform_optimizer (host/test_transform_optimizer on a map file of two keyframes) against the flat Python call on
    the arrays the host filter of transform_optimizer.cc:64-94 leaves: 30 entries of matched_lms_in_keyfrm_2, of which one is null, one
    is to be erased, one is not observed in keyframe 2, one faces a keypoint of keyframe 1 without a landmark and one faces a landmark of
    keyframe 1 that is to be erased; four of the rest are gross mismatches."""
    exe = ROOT / "stella_vslam_amd" / "host" / "test_transform_optimizer"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    n = 30
    p = T._scene(3, n, T.pinhole(), T.pinhole(480.0, 482.0, 330.0, 250.0), False, T.NUM_ITER, gross=4)
    rng = np.random.default_rng(5)
    oct1, oct2 = rng.integers(0, 4, n), rng.integers(0, 4, n)
    inv = _orb_inv_level_sigma_sq()
    obs1, obs2 = p["obs1"].astype(np.float32).astype(np.float64), p["obs2"].astype(np.float32).astype(np.float64)  # cv::KeyPoint holds floats
    idx2 = n - 1 - np.arange(n)
    null, erased2, unobserved, no_lm1, erased1 = 2, 6, 11, 17, 21
    f = lambda v: " ".join(repr(float(x)) for x in v)
    cam = lambda c: f"{c['model']} {int(c['cols'])} {int(c['rows'])} {f([c['fx'], c['fy'], c['cx'], c['cy']])}"
    lines = [f"0 {p['num_iter']} {float(p['chi_sq'])!r}", cam(p["cam1"]) + " " + f(p["pose1"]), cam(p["cam2"]) + " " + f(p["pose2"]), f(p["sim3"]), str(n)]
    lines += [f"{f(obs1[k])} {oct1[k]} {int(k != no_lm1)} {int(k == erased1)} {f(p['pos1'][k])}" for k in range(n)]
    lines.append(str(n))
    at2 = np.argsort(idx2)  # keypoint j of keyframe 2 belongs to match at2[j]
    lines += [f"{f(obs2[at2[j]])} {oct2[at2[j]]}" for j in range(n)]
    lines += [f"{int(k != null)} {int(k == erased2)} {-1 if k == unobserved else idx2[k]} {f(p['pos2'][k])}" for k in range(n)]
    path = tmp_path / "pair.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}
    got_ret, got_sim3, got_null = int(rows["RET"][0]), np.array(rows["SIM3"], np.float64), np.array(rows["NULL"], int)
    # the flat call on the filtered arrays, in ascending idx1 order
    keep = np.array([k for k in range(n) if k not in (null, erased2, unobserved, no_lm1, erased1)])
    from stella_vslam_amd import optimize
    v1, v2 = _views(p)
    flat = optimize.sim3_transform_optimize(ctx, v1, v2, obs1[keep], obs2[keep], inv[oct1[keep]], inv[oct2[keep]], p["pos1"][keep], p["pos2"][keep], p["sim3"],
                                            chi_sq=float(p["chi_sq"]), fix_scale=False, num_iter=p["num_iter"])
    q = dict(p, obs1=obs1[keep], obs2=obs2[keep], w1=inv[oct1[keep]], w2=inv[oct2[keep]], pos1=p["pos1"][keep], pos2=p["pos2"][keep])
    two_form = T.deviation(np.asarray(T.optimize(q, np.float64)["sim3"], np.float64)[None], np.asarray(T.optimize(q, np.longdouble)["sim3"])[None])
    bound = 16.0 * max(two_form, T.common_floor())
    exp_null = np.zeros(n, int)
    exp_null[null] = 1                                  # came as null; the other filtered entries stay as they came
    exp_null[keep[flat["status"] != 0]] = 1
    dev = T.deviation(got_sim3[None], flat["sim3"][None])
    print(f"drop-in: return {got_ret} / {flat['num_inliers']}, Sim3 {dev:.2e} (bound {bound:.2e}), nulls {int(got_null.sum())}, stats {rows['STATS']}")
    assert got_ret == flat["num_inliers"] == len(keep) - 4
    assert np.array_equal(got_null, exp_null) and exp_null[keep[-4:]].all()
    assert dev <= bound
    assert [int(v) for v in rows["STATS"]] == [*flat["lm_iterations"], *flat["lm_trials"], flat["early_return"], flat["num_survivors"]]


def test_host_program_of_the_drop_in_class():
    exe = ROOT / "stella_vslam_amd" / "host" / "test_transform_optimizer"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "transform_optimizer ok" in out.stdout
