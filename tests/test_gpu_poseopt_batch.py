"""svgpu_pose_optimize_batch: every problem of a batch comes back bit for bit as svgpu_pose_optimize returns it for the problem's selected
entries, whatever else the batch holds and wherever the problem stands in it; against the CPU oracle with the project's 1e-4 (TOL and _rel
of tests/test_gpu_ba.py).  The problems are the classes of tests/poseopt_batch_problems.py, all of one camera in one batch."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import pnp_problems as PP
from tests import poseopt_batch_problems as PB
from tests.test_gpu_ba import TOL, _rel

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CALLS = ("perspective", "stereo", "equirect")


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


def _optimizer(ctx, reset):
    from stella_vslam_amd import optimize
    return optimize.pose_optimizer(ctx=ctx, reset_stop_flag_each_round=reset)  # the default trial counts 2 / 2 / 10


def _run(po, problems, **kw):
    b = PB.batch(problems, **kw)
    nv, pose, outl, it = po.optimize_batch_flat(b["poses_cw"], b["obs_off"], b["pos_w"], b["uvr"], b["inv_sigma_sq"], b["huber"], b["intr"], select=b["select"],
                                                active=b["active"])
    off = b["obs_off"]
    return [(int(nv[p]), pose[p].copy(), outl[off[p]:off[p + 1]].copy(), int(it[p])) for p in range(len(problems))]


_REFERENCE = {}


def _reference(ctx, call, reset):
    """per problem of a call: (what svgpu_pose_optimize gives for the selected entries, what the oracle gives, what the big batch gives) --
    computed once, shared by the tests, never changed"""
    key = (call, reset)
    if key not in _REFERENCE:
        po = _optimizer(ctx, reset)
        single, oracle = [], []
        for p in PB.classes()[call]:
            s = PB.selected(p)
            single.append(po.optimize_flat(s["pose_cw"], s["pos_w"], s["uvr"], s["inv_sigma_sq"], s["huber"], s["intr"]))
            oracle.append(O.pose_optimize(s["pose_cw"], s["pos_w"], s["uvr"], s["inv_sigma_sq"], s["huber"], s["intr"], reset_flag_each_round=reset))
        _REFERENCE[key] = (single, oracle, _run(po, PB.classes()[call]))
    return _REFERENCE[key]


def _same(a, b):
    return a[0] == b[0] and a[3] == b[3] and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("call", CALLS)
def test_every_problem_of_a_batch_equals_the_single_call_and_the_oracle(ctx, call, reset):
    problems = PB.classes()[call]
    single, oracle, got = _reference(ctx, call, reset)
    for p, (nv1, pose1, outl1, it1), (nvo, poseo, outlo, sto), (nv, pose, flags, it) in zip(problems, single, oracle, got):
        keep = PB.selected(p)["keep"]
        active = p["active"]
        assert len(flags) == len(keep)
        assert not flags[~keep].any(), p["name"]                     # an unselected entry is never flagged
        if PB.is_skipped(p):
            assert nv == 0 and it == 0 and not flags.any(), p["name"]
            assert pose.tobytes() == p["pose_cw"].tobytes(), p["name"]  # the input pose, bit for bit
            if active:
                assert nv1 == 0 and it1 == 0 and nvo == 0
            continue
        # bit for bit what svgpu_pose_optimize gives for the selected entries
        assert nv == nv1 and it == it1, (p["name"], nv, nv1, it, it1)
        assert pose.tobytes() == np.asarray(pose1).tobytes(), p["name"]
        assert np.array_equal(flags[keep], outl1), p["name"]
        # the oracle: same schedule, same classification, the pose within the project's tolerance
        err = _rel(pose, poseo)
        print(f"{call} reset={reset} {p['name']}: n {int(keep.sum())} num_valid {nv} / {nvo} iterations {it} / {int(sto[0])} rel {err:.3e}")
        assert it == int(sto[0]) and nv == nvo, p["name"]
        assert np.array_equal(flags[keep], outlo), p["name"]
        assert err < TOL, p["name"]


@pytest.mark.parametrize("call", CALLS)
def test_reversed_batch_gives_the_reversed_results(ctx, call):
    got = _reference(ctx, call, False)[2]
    rev = _run(_optimizer(ctx, False), PB.classes()[call][::-1])
    assert len(rev) == len(got)
    for a, b in zip(got, rev[::-1]):
        assert _same(a, b)


def test_a_batch_of_one_equals_the_problem_in_the_big_batch(ctx):
    po = _optimizer(ctx, False)
    for call in CALLS:
        got = _reference(ctx, call, False)[2]
        for p, g in zip(PB.classes()[call], got):
            assert _same(_run(po, [p])[0], g), p["name"]


def test_null_select_and_null_active_mean_all(ctx):
    po = _optimizer(ctx, False)
    names = ("size_65", "size_4", "size_513", "size_0", "size_5")
    problems = [p for p in PB.classes()["perspective"] if p["name"] in names]
    got = {p["name"]: g for p, g in zip(PB.classes()["perspective"], _reference(ctx, "perspective", False)[2])}
    for kw in (dict(with_select=False), dict(with_active=False), dict(with_select=False, with_active=False)):
        for p, r in zip(problems, _run(po, problems, **kw)):
            assert _same(r, got[p["name"]]), (p["name"], kw)


def test_two_calls_are_bit_equal(ctx):
    again = _run(_optimizer(ctx, False), PB.classes()["perspective"])
    for a, b in zip(_reference(ctx, "perspective", False)[2], again):
        assert _same(a, b)


def test_more_workgroups_than_compute_units(ctx):
    """300 copies of the 65-entry problem: more workgroups than the 256 CUs hold at one per CU, each tiny -- 300 identical results."""
    p = next(q for q in PB.classes()["perspective"] if q["name"] == "size_65")
    one = next(g for q, g in zip(PB.classes()["perspective"], _reference(ctx, "perspective", False)[2]) if q["name"] == "size_65")
    got = _run(_optimizer(ctx, False), [p] * 300)
    assert len(got) == 300 and one[3] > 0
    for g in got:
        assert _same(g, one)


def test_chain_from_pnp_ransac_batch(ctx):
    """svgpu_pnp_ransac_batch on three candidates, one of them invalid: its pose_cw, valid and is_inlier go straight in as pose_cw, active
    and select; the result is what compacting on the host and one optimize_flat per valid candidate give."""
    from stella_vslam_amd import solve
    cands = [PP.planted(71, 80, "pinhole", noise=2e-3, outliers=0.2), PP.planted(72, 3, "pinhole"), PP.planted(73, 120, "pinhole", noise=2e-3, outliers=0.2)]
    off, brg, pw, octv = PP.concatenate(cands)
    sf = cands[0]["scale_factors"]
    samples = np.stack([PP.draw_samples(np.random.default_rng(170 + j), len(c["pos_w"]), 30) for j, c in enumerate(cands)])
    pnp = solve.pnp_ransac_batch(ctx, off, brg, pw, octv, sf, samples)
    assert list(pnp["valid"]) == [1, 0, 1]
    # the current frame's observations of the matches: a pinhole camera, the octave's sigma, the monocular Huber width
    K = np.array([458.654, 457.296, 367.215, 248.375, 0.0])
    uvr = np.stack([K[0] * brg[:, 0] / brg[:, 2] + K[2], K[1] * brg[:, 1] / brg[:, 2] + K[3], -np.ones(len(brg))], 1).astype(np.float32)
    w = (1.0 / np.asarray(sf, np.float32)[octv] ** 2).astype(np.float32)
    hub = np.full(len(brg), np.sqrt(np.float32(5.99146)), np.float32)
    po = _optimizer(ctx, False)
    nv, pose, flags, it = po.optimize_batch_flat(pnp["pose_cw"], off, pw, uvr, w, hub, K, select=pnp["is_inlier"], active=pnp["valid"])
    for c in range(3):
        sl = slice(off[c], off[c + 1])
        keep = pnp["is_inlier"][sl] != 0
        if not pnp["valid"][c]:
            assert nv[c] == 0 and it[c] == 0 and not flags[sl].any() and pose[c].tobytes() == pnp["pose_cw"][c].tobytes()
            continue
        assert keep.sum() >= 50
        nv1, pose1, outl1, it1 = po.optimize_flat(pnp["pose_cw"][c], pw[sl][keep], uvr[sl][keep], w[sl][keep], hub[sl][keep], K)
        assert nv[c] == nv1 and it[c] == it1 and it1 > 0 and pose[c].tobytes() == pose1.tobytes()
        assert np.array_equal(flags[sl][keep], outl1) and not flags[sl][~keep].any()
        assert nv1 >= 0.8 * keep.sum()


def _raw(ctx, **over):
    """the C entry point with valid arguments of a two-problem batch, any of them replaced; returns (status, error string, pose_out)"""
    from stella_vslam_amd._lib import lib
    problems = [p for p in PB.classes()["perspective"] if p["name"] in ("size_5", "size_65")]
    b = PB.batch(problems)
    out, outl = np.full((2, 12), -7.0), np.zeros(len(b["pos_w"]), np.uint8)
    nv, it = np.full(2, -7, np.int32), np.full(2, -7, np.int32)
    a = dict(num_problems=2, obs_off=b["obs_off"], pose_cw=b["poses_cw"], active=b["active"], pos_w=b["pos_w"], uvr=b["uvr"], inv_sigma_sq=b["inv_sigma_sq"],
             huber=b["huber"], select=b["select"], intr=b["intr"], num_trials_robust=2, num_trials=2, num_each_iter=10, reset=0, pose_out=out, flags=outl,
             num_valid=nv, lm_iterations=it)
    a.update(over)
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    L = lib()
    rc = L.svgpu_pose_optimize_batch(a.get("handle", ctx.handle), a["num_problems"], vp(a["obs_off"]), vp(a["pose_cw"]), vp(a["active"]), vp(a["pos_w"]), vp(a["uvr"]),
                                     vp(a["inv_sigma_sq"]), vp(a["huber"]), vp(a["select"]), vp(a["intr"]), a["num_trials_robust"], a["num_trials"],
                                     a["num_each_iter"], a["reset"], vp(a["pose_out"]), vp(a["flags"]), vp(a["num_valid"]), vp(a["lm_iterations"]))
    return rc, L.svgpu_last_error(ctx.handle).decode(), out, nv


INVALID = [dict(obs_off=np.array([0, 70, 5], np.int32)), dict(obs_off=np.array([1, 5, 70], np.int32)), dict(obs_off=None), dict(pose_cw=None), dict(pos_w=None),
           dict(uvr=None), dict(inv_sigma_sq=None), dict(huber=None), dict(intr=None), dict(pose_out=None), dict(flags=None), dict(num_valid=None),
           dict(num_trials_robust=-1), dict(num_trials=-1), dict(num_each_iter=-1), dict(num_problems=-1)]


@pytest.mark.parametrize("over", INVALID, ids=lambda o: next(iter(o)) + ("" if next(iter(o.values())) is None else "_bad"))
def test_invalid_arguments_return_before_anything_is_launched(ctx, over):
    from stella_vslam_amd._lib import lib
    L = lib()
    assert L.svgpu_profile_select(ctx.handle, b"k_pose_opt_batch") == 0
    try:
        rc, msg, out, nv = _raw(ctx, **over)
        ms, launches = C.c_double(0), C.c_longlong(0)
        assert L.svgpu_profile_read_class(ctx.handle, b"k_pose_opt_batch", C.byref(ms), C.byref(launches)) == 0
    finally:
        L.svgpu_profile_select(ctx.handle, None)
    assert rc == 1 and "svgpu_pose_optimize_batch" in msg, (rc, msg)
    assert launches.value == 0
    assert (out == -7.0).all() and (nv == -7).all()  # no output was touched


def test_valid_arguments_of_the_validation_test_succeed_and_launch_once(ctx):
    from stella_vslam_amd._lib import lib
    L = lib()
    assert L.svgpu_profile_select(ctx.handle, b"k_pose_opt_batch") == 0
    try:
        rc, msg, out, nv = _raw(ctx)
        rc2 = _raw(ctx, lm_iterations=None)[0]  # the iteration counts are optional, as in svgpu_pose_optimize
        ms, launches = C.c_double(0), C.c_longlong(0)
        assert L.svgpu_profile_read_class(ctx.handle, b"k_pose_opt_batch", C.byref(ms), C.byref(launches)) == 0
    finally:
        L.svgpu_profile_select(ctx.handle, None)
    assert rc == 0 and rc2 == 0 and launches.value == 2 and ms.value > 0
    assert (nv >= 5).all() and not (out == -7.0).any()


def test_no_problem_succeeds_with_null_pointers_and_a_null_context_is_invalid(ctx):
    from stella_vslam_amd._lib import lib
    L = lib()
    assert L.svgpu_pose_optimize_batch(ctx.handle, 0, *([None] * 9), 2, 2, 10, 0, *([None] * 4)) == 0
    assert L.svgpu_pose_optimize_batch(ctx.handle, 0, *([None] * 9), -1, -1, -1, 0, *([None] * 4)) == 0  # whatever else is passed
    assert _raw(ctx, handle=None)[0] == 1
    nv, pose, outl, it = _optimizer(ctx, False).optimize_batch_flat(np.zeros((0, 12)), [0], np.zeros((0, 3)), np.zeros((0, 3)), [], [], [500, 500, 320, 240, 0])
    assert len(nv) == 0 and pose.shape == (0, 12) and len(outl) == 0 and len(it) == 0


def test_mirror_rejects_disagreeing_lengths(ctx):
    po = _optimizer(ctx, False)
    b = PB.batch([p for p in PB.classes()["perspective"] if p["name"] in ("size_5", "size_65")])
    args = lambda **o: {**dict(poses_cw=b["poses_cw"], obs_off=b["obs_off"], pos_w=b["pos_w"], uvr=b["uvr"], inv_sigma_sq=b["inv_sigma_sq"], huber=b["huber"],
                               intr=b["intr"], select=b["select"], active=b["active"]), **o}
    for bad in (dict(poses_cw=b["poses_cw"][:1]), dict(uvr=b["uvr"][:-1]), dict(inv_sigma_sq=b["inv_sigma_sq"][:-1]), dict(huber=b["huber"][1:]),
                dict(select=b["select"][:-1]), dict(active=b["active"][:1]), dict(obs_off=b["obs_off"][:-1])):
        with pytest.raises(ValueError):
            po.optimize_batch_flat(**args(**bad))


def test_kernel_is_listed_for_profiling():
    from stella_vslam_amd._lib import lib
    L = lib()
    assert "k_pose_opt_batch" in L.svgpu_profile_kernels().decode().split(",")


def test_drop_in_optimize_batch_equals_the_single_overload():
    """host/drop_in/pose_optimizer_hip::optimize_batch over the stand-ins: three candidates (one below 5 landmarks) against three single calls,
    and find_via_ransac_batch -> optimize_batch on two candidates."""
    exe = ROOT / "stella_vslam_amd" / "host" / "test_pose_optimizer_batch"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pose_optimizer batch ok" in out.stdout
