"""The batched bucket matchers on the device: problem p of a batch equals the CPU oracle's answer for its two sides AND the existing
single device call, element for element, counts included -- everything is integer or index work, so the bar is equality."""
import ctypes as C

import numpy as np
import pytest

from tests import bucket_batch_problems as BP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd import feature
    return feature.Context()


def run(ctx, b, ori):
    from stella_vslam_amd import match
    if b["kind"] == "bow":
        return match.bow_tree(b["lowe_ratio"], ori, ctx).match_batch(b["side1"], b["side2"])
    return match.match_for_triangulation_batch(ctx, b["lowe_ratio"], ori, b["side1"], b["side2"], b["E_12"], b["epipole_in_2"], b["valid_epipole"],
                                               b["scale_factors"], b["residual_rad_thr"])


def single_gpu(ctx, b, ori):
    from stella_vslam_amd import match

    def bow(lowe, o, d1, a1, v1, n1, d2, a2, n2, valid2=None, occupied2=None):
        return match.bow_tree(lowe, o, ctx).match(d1, a1, v1, n1, d2, a2, n2, valid2=valid2, occupied2=occupied2)

    def tri(lowe, o, *a, **kw):
        return match.match_for_triangulation(ctx, lowe, o, *a, **kw)
    return [BP.single(b, p, ori, bow, tri) for p in range(BP.num_problems(b))]


def same(got, ref):
    lists, nums = got
    assert len(lists) == len(ref) == len(nums)
    for p, (m, n) in enumerate(ref):
        assert np.array_equal(lists[p], m), p
        assert int(nums[p]) == int(n), p


@pytest.mark.parametrize("ori", [True, False], ids=["ori", "no_ori"])
@pytest.mark.parametrize("name", BP.CLASSES)
def test_batch_equals_oracle_and_single_call(ctx, name, ori):
    b = BP.batch(name)
    if b["kind"] == "tri":
        assert BP.acos_margin(b) > 1e3 or name == "planted_tri"  # no pair within rounding distance of the acos decisions (planted_tri: residual exactly 0)
    got = run(ctx, b, ori)
    same(got, BP.oracle(b, ori))
    same(got, single_gpu(ctx, b, ori))
    if "expect" in b:
        for p, e in enumerate(b["expect"](ori)):
            assert e is None or np.array_equal(got[0][p], e), p
    if name == "reloc":
        assert np.array_equal(got[0][1], got[0][2]) and got[1][1] == got[1][2] > 0  # the same arrays twice: identical lists
    for p in range(len(got[1])):
        assert (got[1][p] == 0) == (p in b["degenerate"]) or name in ("planted_eq", "planted_lo", "planted_hi", "planted_tri"), p


@pytest.mark.parametrize("name", ["reloc", "loop", "unshared", "tri_bow", "planted_eq"])
def test_reversed_unshared_and_batches_of_one(ctx, name):
    b = BP.batch(name)
    lists, nums = run(ctx, b, True)
    rl, rn = run(ctx, BP.reversed_batch(b), True)
    assert np.array_equal(rn[::-1], nums) and all(np.array_equal(a, c) for a, c in zip(rl[::-1], lists))
    ul, un = run(ctx, BP.unshared_batch(b), True)
    assert np.array_equal(un, nums) and all(np.array_equal(a, c) for a, c in zip(ul, lists))
    one = single_gpu(ctx, b, True)
    for p in range(min(BP.num_problems(b), 6)):
        l1, n1 = run(ctx, BP.batch_of_one(b, p), True)
        assert np.array_equal(l1[0], one[p][0]) and int(n1[0]) == int(one[p][1]), p


def test_arena_regrowth_and_reuse():
    from stella_vslam_amd import feature
    c = feature.Context()  # a context of its own: the arena starts small
    for name in ("unshared", "spill", "unshared"):
        b = BP.batch(name)
        same(run(c, b, False), BP.oracle(b, False))


def test_chain_into_triangulation(ctx):
    """The triangulation batch's matches go through triangulation_matches_to_batch into triangulate_two_views_batch and give, per neighbour,
    the bytes of the per-neighbour path: match_for_triangulation, then triangulate_two_views on its pair list."""
    from stella_vslam_amd import match
    from stella_vslam_amd.camera import svgpu_camera
    from tests import match_problems as MP
    from tests import triangulation_problems as T
    sc = MP.scene(seed=7)
    gcam = MP.make_cams(sc, "svgpu")
    kw = MP.triangulation(sc, lambda R, t, c: match.reproject_to_bearing(gcam, R, t, c))
    a, b = sc["views"][0], sc["views"][1]
    n2 = len(kw["desc2"])
    rng = np.random.default_rng(3)
    sels = [np.arange(n2), np.sort(rng.choice(n2, n2 * 2 // 3, replace=False)), np.sort(rng.choice(n2, n2 // 3, replace=False))]
    s1 = dict(desc=kw["desc1"], angle=kw["angle1"], octave=kw["octave1"], bearings=kw["bearings1"], has_lm=kw["has_lm1"])
    s2 = [dict(desc=kw["desc2"][i], angle=kw["angle2"][i], bearings=kw["bearings2"][i], has_lm=kw["has_lm2"][i]) for i in sels]
    k = len(sels)
    E, ep = np.stack([np.asarray(kw["E_12"], np.float64)] * k), np.stack([np.asarray(kw["epipole_in_2"], np.float64)] * k)
    lists, nums = match.match_for_triangulation_batch(ctx, 0.8, True, s1, s2, E, ep, np.full(k, int(kw["valid_epipole"]), np.int32), kw["scale_factors"],
                                                      kw["residual_rad_thr"])
    assert nums.sum() > 40 and (nums > 0).all()
    off, i1, i2 = match.triangulation_matches_to_batch(lists)
    assert off.dtype == np.int32 and i1.dtype == np.int32 and i2.dtype == np.int32 and off[-1] == nums.sum()

    fx, fy, cx, cy, fxb = sc["K"]
    cam = T.camera(T.PERSPECTIVE, cols=sc["width"], rows=sc["height"], fx=fx, fy=fy, cx=cx, cy=cy, true_baseline=fxb / fx)
    c = svgpu_camera()
    c.model, c.cols, c.rows, c.fx, c.fy, c.cx, c.cy = cam["model"], cam["cols"], cam["rows"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    c.focal_x_baseline = cam["focal_x_baseline"]
    c.min_x, c.max_x, c.min_y, c.max_y = cam["bounds"]
    tb = dict(T.orb_tables(), scale_factors=np.asarray(sc["tables"]["scale_factors"], np.float32))
    tb["level_sigma_sq"] = (tb["scale_factors"] * tb["scale_factors"]).astype(np.float32)

    def view(v, brg, sel):
        pose = np.concatenate([np.asarray(v["rot_cw"], np.float64), np.asarray(v["trans_cw"], np.float64)[:, None]], 1)
        return dict(cam=c, pose_cw=pose, true_baseline=cam["true_baseline"], xy=np.asarray(v["xy"], np.float32)[sel], octave=np.asarray(v["octave"], np.int32)[sel],
                    bearings=np.asarray(brg, np.float64)[sel], xright=None, depth=None, scale_factor=tb["scale_factor"])
    g1 = view(a, kw["bearings1"], np.arange(len(kw["desc1"])))
    gn = [view(b, kw["bearings2"], i) for i in sels]
    pos, st, acc = match.triangulate_two_views_batch(ctx, g1, gn, off, tb["scale_factors"], tb["level_sigma_sq"], i1, i2)
    assert (st == T.ACCEPTED).sum() > 20
    for j in range(k):  # the per-neighbour path: one matcher call, one triangulator call
        m21, num = match.match_for_triangulation(ctx, 0.8, True, **dict(kw, desc2=s2[j]["desc"], angle2=s2[j]["angle"], bearings2=s2[j]["bearings"],
                                                                        has_lm2=s2[j]["has_lm"]))
        has = m21 >= 0
        ps, ss, ns = match.triangulate_two_views(ctx, g1, gn[j], tb["scale_factors"], tb["level_sigma_sq"], np.flatnonzero(has), m21[has])
        lo, hi = off[j], off[j + 1]
        assert num == nums[j] == hi - lo and np.array_equal(ss, st[lo:hi]) and ns == acc[j], j
        assert ps.tobytes() == pos[lo:hi].tobytes(), j


def test_drop_in_batch_methods_equal_the_per_call_methods():
    """host/test_bucket_batch: bow_tree::match_frame_and_keyframe_batch / match_keyframes_batch / match_for_triangulation_batch (and robust's)
    beside the per-call methods on identical stand-in objects."""
    import pathlib
    import subprocess
    exe = pathlib.Path(__file__).resolve().parent.parent / "stella_vslam_amd" / "host" / "test_bucket_batch"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bucket batch drop-in ok" in out.stdout


def _view(match, side):
    keep = []
    return match._match_view(side, keep), keep


def test_invalid_arguments_then_a_valid_call(ctx):
    from stella_vslam_amd import match
    from stella_vslam_amd._lib import lib, ptr
    L = lib()
    b = BP.batch("unshared")
    s1, s2 = BP.sides(b, 1)
    tb = BP.batch("planted_tri")
    t1, t2 = BP.sides(tb, 0)
    out, num = np.full(4096, -1, np.int32), np.zeros(8, np.int32)
    E, ep, ve, sf = np.zeros(18), np.zeros(6), np.zeros(2, np.int32), np.ones(2, np.float32)

    def bow(a, c, k=1, sh1=0, sh2=0, ori=1, o=out, n=num):
        keep = []
        va = (match.svgpu_match_view * max(len(a), 1))(*[match._match_view(x, keep) for x in a]) if a is not None else None
        vc = (match.svgpu_match_view * max(len(c), 1))(*[match._match_view(x, keep) for x in c]) if c is not None else None
        return va, vc, lambda: L.svgpu_bow_match_batch(ctx.handle, k, va, sh1, vc, sh2, 0.75, ori, ptr(o), ptr(n))

    def tri(a, c, levels=2, ori=1, e=E):
        keep = []
        va, vc = match._match_view(a, keep), match._match_view(c, keep)
        return va, vc, lambda: L.svgpu_match_for_triangulation_batch(ctx.handle, 1, C.byref(va), 0, C.byref(vc), 0, ptr(e), ptr(ep), ptr(ve), ptr(sf), levels,
                                                                     0.01, 0.8, ori, ptr(out), ptr(num))
    drop = lambda s, k: {x: (None if x == k else v) for x, v in s.items()}  # noqa: E731
    calls = {
        "null side": bow(None, [s2]), "null output": bow([s1], [s2], o=None), "null counts": bow([s1], [s2], n=None),
        "node on one side": bow([s1], [drop(s2, "node")]), "no node on side 1": bow([drop(s1, "node")], [drop(s2, "node")]),
        "orientation without angles": bow([drop(s1, "angle")], [s2]), "orientation without angles 2": bow([s1], [drop(s2, "angle")]),
        "occupied on side 1": bow([dict(s1, occupied=np.zeros(len(s1["desc"]), np.uint8))], [s2]),
        "both shared": bow([s1], [s2], k=2, sh1=1, sh2=1), "negative problems": bow([s1], [s2], k=-1),
        "no bearings": tri(drop(t1, "bearings"), t2), "no bearings 2": tri(t1, drop(t2, "bearings")), "no octave": tri(drop(t1, "octave"), t2),
        "levels 0": tri(t1, t2, levels=0), "levels 17": tri(t1, t2, levels=17), "octave out of range": tri(dict(t1, octave=np.full(len(t1["desc"]), 2, np.int32)), t2),
        "negative octave": tri(dict(t1, octave=np.full(len(t1["desc"]), -1, np.int32)), t2), "no E": tri(t1, t2, e=None),
        "occupied in triangulation": tri(t1, dict(t2, occupied=np.zeros(len(t2["desc"]), np.uint8))),
    }
    for what, (va, vc, call) in calls.items():
        assert call() == 1, what  # SVGPU_ERR_INVALID
        assert L.svgpu_last_error(ctx.handle), what
    va, vc, call = bow([s1], [s2])
    va[0].n = -1
    assert call() == 1
    va[0].n, vc[0].n = len(s1["desc"]), 1 << 22
    assert call() == 1
    vc[0].n = len(s2["desc"])
    # element totals beyond int32: two problems of (1 << 22) - 1 keypoints a side, side 2 shared -- the sum of n1 x n2 does not fit; the
    # check comes before any array is read (the arrays behind these views are far shorter)
    va2, vc2, big = bow([s1, s1], [s2], k=2, sh2=1)
    va2[0].n = va2[1].n = vc2[0].n = (1 << 22) - 1
    assert big() == 1
    assert call() == 0  # a valid call on the same context
    same(run(ctx, b, True), BP.oracle(b, True))
    assert L.svgpu_bow_match_batch(ctx.handle, 0, None, 0, None, 0, 0.75, 1, None, None) == 0  # num_problems == 0 succeeds whatever else is passed


def test_profile_classes_listed():
    from stella_vslam_amd._lib import lib
    names = lib().svgpu_profile_kernels().decode().split(",")
    assert "k_bucket_batch" in names and "k_cand_batch" in names
