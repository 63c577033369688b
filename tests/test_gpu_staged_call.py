"""The staged call (csrc/sv_staged_call.h) owns the regrowth of the scratch arena and of its page-locked mirror.  On ONE context two cheap
entry points are called small -> large -> small, the large call past the 1 MiB scratch granule and the first stage buffer, so both buffers
are replaced between calls; every output has to be bit-equal to the same call made on a fresh context.  Then the zero-filled mirror
path of svgpu_match_bruteforce (no angle arrays: the rows are written in the mirror, not uploaded) against the oracle.
The same small -> large -> small round for the entry points that joined the protocol later (Hamming distances, the landmark refresh,
the BoW descent, the frame observation, the landmark table's upsert / erase / download), and the frame observation's cell_items
read-back: the whole piece comes back with the other results, the caller's array receives cell_off[last] entries and not one more."""
import ctypes as C

import numpy as np
import pytest

from tests import pnp_problems as PNP
from tests import posegraph_problems as PG

pytestmark = pytest.mark.gpu


def _context():
    from stella_vslam_amd.feature import Context
    return Context()


def _same_on_fresh_contexts(call, problems):
    shared = _context()
    for k, p in enumerate(problems):
        got, exp = call(shared, p), call(_context(), p)
        for g, e in zip(got, exp):
            assert g.shape == e.shape and g.tobytes() == e.tobytes(), f"call {k}"


def test_landmark_correction_small_large_small():
    from stella_vslam_amd import optimize
    before = np.stack([PG.make_sim3([0.1, -0.2, 0.3], [1.0, 2.0, 3.0], 1.0), PG.make_sim3([-0.3, 0.1, 0.2], [-2.0, 0.5, 1.0], 1.5)])
    after = np.stack([before[0], PG.make_sim3([-0.25, 0.15, 0.2], [-2.1, 0.4, 1.2], 1.4)])

    def problem(L):  # about 52 bytes of arena per landmark: 40 000 of them take some 2 MB
        rng = np.random.default_rng(L)
        return rng.integers(0, 2, size=L).astype(np.int32), rng.normal(size=(L, 3)) * 10.0

    def call(ctx, p):
        return (optimize.correct_landmarks(ctx, before, after, p[0], p[1]),)

    problems = [problem(1), problem(40000), problem(1)]
    _same_on_fresh_contexts(call, problems)
    ref, pos = problems[1]  # and the large call computes what numpy computes
    out = call(_context(), problems[1])[0]
    exp = PG.correct_landmarks(before.astype(np.longdouble), after.astype(np.longdouble), ref, pos.astype(np.longdouble))
    assert float((np.abs(out - exp).max(1) / np.maximum(1.0, np.abs(exp).max(1))).max()) <= 1e-12


def test_pnp_pose_small_large_small():
    from stella_vslam_amd import solve
    one = [PNP.planted(7, 4, "pinhole")]
    many = [PNP.planted(100 + s, 12, PNP.KINDS[s % 4], noise=1e-3) for s in range(2000)]

    def call(ctx, sets):
        off, brg, pw, _ = PNP.concatenate(sets)
        return solve.compute_pose(ctx, brg, pw, off)

    _same_on_fresh_contexts(call, [one, many, one])


def test_bruteforce_without_angle_arrays_against_the_oracle():
    from oracle import oracle as O
    from stella_vslam_amd import match
    rng = np.random.default_rng(5)
    n = 64
    d1 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    d2 = d1[rng.permutation(n)].copy()
    flips = rng.integers(0, 256, size=(n, 3))  # three flipped bits per descriptor: unambiguous nearest neighbours
    for i in range(n):
        for b in flips[i]:
            d2[i, b // 8] ^= np.uint8(1 << (b % 8))
    pairs, out = match.robust(0.8, False, _context()).brute_force_match(d1, None, d2, None)
    zeros = np.zeros(n, np.float32)
    exp = O.brute_force_match(d1, zeros, d2, zeros, None, 0.8, False)
    assert np.array_equal(out, exp)
    assert len(pairs) == int((exp >= 0).sum()) > n // 2


def test_hamming_small_large_small():
    from oracle import oracle as O
    from stella_vslam_amd import match

    def problem(n, seed):  # 68 bytes of arena per row pair: 20 000 of them pass the 1 MiB granule
        rng = np.random.default_rng(seed)
        return rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)

    def pairs(ctx, p):
        return (match.compute_descriptor_distance_32(ctx, p[0], p[1]),)

    def matrix(ctx, p):  # the n1 x n2 matrix lies behind both descriptor arrays
        return (match.hamming_matrix(ctx, p[0], p[1][: max(1, len(p[1]) // 50)]),)

    problems = [problem(1, 0), problem(20000, 1), problem(1, 2)]
    _same_on_fresh_contexts(pairs, problems)
    _same_on_fresh_contexts(matrix, problems)
    a, b = problems[1]
    assert np.array_equal(pairs(_context(), problems[1])[0], np.unpackbits(a ^ b, axis=1).sum(1))
    assert np.array_equal(matrix(_context(), problems[1])[0], O.hamming_matrix(a, b[:400]))


def test_landmark_refresh_small_large_small():
    from oracle import oracle as O
    from stella_vslam_amd import data
    from tests.test_oracle_landmark import _scene

    def descriptor_problem(n, seed):  # some 38 bytes per observation and 40 per landmark: 8 000 landmarks of ~4.3 observations take 1.7 MB
        rng = np.random.default_rng(seed)
        return _scene(rng, n) if n > 1 else (np.array([0, 1], np.int32), rng.integers(0, 256, (1, 32), dtype=np.uint8))

    def geometry_problem(n, seed):  # 24 bytes per observation and 88 per landmark
        rng = np.random.default_rng(seed)
        k = rng.integers(1, 12, n) if n > 1 else np.array([1])
        off = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
        pos = rng.uniform(-5, 5, (n, 3))
        cams = np.repeat(pos, k, axis=0) + rng.normal(0, 4.0, (off[-1], 3))
        ref = cams[off[:-1] + rng.integers(0, k)]
        sf = np.float32(1.2) ** rng.integers(0, 8, n).astype(np.float32)
        return off, cams, pos, ref, sf, float(np.float32(1.0) / np.float32(1.2) ** np.float32(7))

    dp = [descriptor_problem(1, 0), descriptor_problem(8000, 1), descriptor_problem(1, 2)]
    gp = [geometry_problem(1, 3), geometry_problem(8000, 4), geometry_problem(1, 5)]
    _same_on_fresh_contexts(lambda ctx, p: data.landmarks_compute_descriptor(ctx, *p), dp)
    _same_on_fresh_contexts(lambda ctx, p: data.landmarks_update_mean_normal_and_obs_scale_variance(ctx, *p), gp)
    # one context through both entry points in turn, against the oracle
    ctx = _context()
    for d, g in zip(dp, gp):
        for got, exp in zip(data.landmarks_compute_descriptor(ctx, *d), O.landmarks_compute_descriptor(*d)):
            assert np.array_equal(got, exp)
        for got, exp in zip(data.landmarks_update_mean_normal_and_obs_scale_variance(ctx, *g), O.landmarks_update_geometry(*g)):
            assert np.array_equal(got, exp)


def test_bow_transform_small_large_small():
    from oracle import oracle as O
    from stella_vslam_amd import data
    from tests.test_oracle_bow import make_tree
    tree = make_tree(np.random.default_rng(1), k=10, depth=3, prune=0.05)
    leaves = np.flatnonzero(tree["word_id"] >= 0)

    def problem(n, seed):  # 44 bytes of arena per descriptor: 30 000 of them pass the granule
        rng = np.random.default_rng(seed)
        q = tree["node_desc"][rng.choice(leaves, n)].copy()
        q[::7] = rng.integers(0, 256, (len(q[::7]), 32), dtype=np.uint8)
        return q

    def call(ctx, q):
        voc = data.bow_vocabulary(ctx, tree["child_off"], tree["children"], tree["node_desc"], tree["node_weight"], tree["word_id"], depth=3, k=10)
        return voc.descend(q, 1) + voc.descend_fbow(q, 2)

    problems = [problem(1, 0), problem(30000, 1), problem(1, 2)]
    _same_on_fresh_contexts(call, problems)
    got = call(_context(), problems[1])
    for g, e in zip(got, O.bow_transform(tree, problems[1], 2) + O.fbow_transform(tree, problems[1], 2, 10)):
        assert np.array_equal(g, e)


def test_landmark_table_small_large_small():
    """upsert / erase / download of svgpu_map on one context: 1 id, enough ids to pass the granule (100 bytes of arena each), a batch
    with repeated ids (the host collapses them in the mirror: last entry wins, fewer records travel than were passed), 1 id."""
    from stella_vslam_amd import tracking

    def problem(n, seed, span):
        rng = np.random.default_rng(seed)
        ids = (rng.permutation(span)[:n] if span >= n else rng.integers(0, span, n)).astype(np.uint32)
        rec = tracking.landmark_records(rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), rng.uniform(0.1, 1, n), rng.uniform(1, 9, n),
                                        rng.integers(0, 256, (n, 32), dtype=np.uint8))
        rec["reserved"] = np.arange(n)
        return ids, rec

    def expected(p):
        ids, rec = p
        last = {int(i): k for k, i in enumerate(ids)}  # the last entry of an id wins
        ask = np.array(sorted(last) + [int(ids.max()) + 1, 1 << 29], np.uint32)  # and two ids the table does not hold: zero records
        exp = np.zeros(len(ask), tracking.LANDMARK_RECORD_DTYPE)
        exp[: len(last)] = rec[[last[int(i)] for i in ask[: len(last)]]]
        gone = ask[: len(last)][::3]
        exp["flags"][: len(last)][::3] = 0
        return ask, gone, exp

    def call(ctx, p):
        ask, gone, _ = expected(p)
        table = tracking.landmark_table(ctx)
        try:
            table.upsert(p[0], p[1])
            before = table.download(ask)
            table.erase(gone)
            return before.view(np.uint8), table.download(ask).view(np.uint8)
        finally:
            table.close()

    problems = [problem(1, 0, 10), problem(12000, 1, 12000), problem(1, 2, 10), problem(300, 3, 40), problem(1, 4, 10)]
    assert len(set(problems[3][0].tolist())) < 41
    _same_on_fresh_contexts(call, problems)
    ctx = _context()
    for p in problems:
        _, _, exp = expected(p)
        assert call(ctx, p)[1].tobytes() == exp.tobytes()


def _grid_call(ctx, cam, kps, cols, rows, undist, bearings, off, items):
    from stella_vslam_amd._lib import lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ctx.check(lib().svgpu_frame_observation(ctx.handle, C.byref(cam.c_), p(kps), len(kps), cols, rows, p(undist), p(bearings), p(off), p(items)),
              "svgpu_frame_observation")


def test_frame_observation_cell_items_tail_and_small_large_small():
    from oracle import oracle as O
    from stella_vslam_amd import camera
    ctx = _context()
    cam = camera.equirectangular("theta", "RGB", 1920, 960, 30.0, ctx=ctx)  # undistortion = identity
    bounds = cam.img_bounds_.as_tuple()
    SENTINEL = 0x5A5A5A5A

    def keypoints(n, seed, outside):
        rng = np.random.default_rng(seed)
        k = np.zeros(n, O.KEYPOINT_DTYPE)
        k["x"], k["y"], k["size"], k["class_id"] = rng.uniform(0, 1920, n), rng.uniform(0, 960, n), 31.0, -1
        out = rng.permutation(n)[:outside]  # beyond the bounds on either side: in no cell
        k["x"][out[::2]], k["y"][out[1::2]] = rng.uniform(-90, -1, len(out[::2])), rng.uniform(961, 1100, len(out[1::2]))
        return k

    def observe(c, k, want_items=True, want_rest=True):
        n = len(k)
        und, brg = (np.zeros(n, O.KEYPOINT_DTYPE), np.zeros((n, 3))) if want_rest else (None, None)
        off = np.full(64 * 48 + 1, -7, np.int32)
        items = np.full(n, SENTINEL, np.int32) if want_items else None
        _grid_call(c, cam, k, 64, 48, und, brg, off, items)
        return und, brg, off, items

    k = keypoints(700, 11, 150)
    exp_off, exp_items = O.assign_keypoints_to_grid(k["x"], k["y"], bounds, 64, 48)
    und, brg, off, items = observe(ctx, k)
    last = int(off[-1])
    assert last == exp_off[-1] and 0 < last <= 700 - 150
    assert np.array_equal(off, exp_off) and np.array_equal(items[:last], exp_items[:last])
    assert (items[last:] == SENTINEL).all()  # the header promises cell_off[last] entries and nothing beyond
    assert np.array_equal(und["x"], k["x"]) and np.array_equal(und["y"], k["y"])
    assert np.array_equal(observe(ctx, k, want_items=False)[2], exp_off)
    _, _, off2, items2 = observe(ctx, k, want_rest=False)
    assert np.array_equal(off2, exp_off) and np.array_equal(items2[:last], exp_items[:last]) and (items2[last:] == SENTINEL).all()

    # 100 bytes of arena per keypoint: 20 000 pass the granule (and the one-launch grid build's limit of 8 192)
    def call(c, kp):
        return tuple(a.view(np.uint8) if a.dtype.fields else a for a in observe(c, kp))

    problems = [keypoints(1, 0, 0), keypoints(20000, 1, 3000), keypoints(2, 2, 1)]
    _same_on_fresh_contexts(call, problems)
    off, items = O.assign_keypoints_to_grid(problems[1]["x"], problems[1]["y"], bounds, 64, 48)
    got = observe(_context(), problems[1])
    assert np.array_equal(got[2], off) and np.array_equal(got[3][: off[-1]], items[: off[-1]]) and (got[3][off[-1]:] == SENTINEL).all()
