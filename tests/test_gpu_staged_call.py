"""The staged call (csrc/sv_staged_call.h) owns the regrowth of the scratch arena and of its page-locked mirror.  On ONE context two cheap
entry points are called small -> large -> small, the large call past the 1 MiB scratch granule and the first stage buffer, so both buffers
are replaced between calls; every output has to be bit-equal to the same call made on a fresh context.  Then the zero-filled mirror
path of svgpu_match_bruteforce (no angle arrays: the rows are written in the mirror, not uploaded) against the oracle.
The same small -> large -> small round for the entry points that joined the protocol later (Hamming distances, the landmark refresh,
the BoW descent, the frame observation, the landmark table's upsert / erase / download), and the frame observation's cell_items
read-back: the whole piece comes back with the other results, the caller's array receives cell_off[last] entries and not one more.
Last, the two-pass matchers (in_cells_core, bucket_match): a fresh context sizes the candidate lists exactly, with a read-back of the
total in the middle of the call, a context that has matched before guesses their capacity -- so the same round also compares the two; a guess
that falls short with and without regrowth of the arena, no candidate at all, and a bound resident frame."""
import types

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


# ---- the two-pass matchers.  640 x 480 image, 64 x 48 grid; keypoints uniform over the image with octaves 2..4, so that a query of level 3
# sees all of them inside its window.  Queries sit on keypoints, their descriptors a few bits away.
BOUNDS = (0.0, 640.0, 0.0, 480.0)
FX, CX, CY = 500.0, 320.0, 240.0


def _keypoints(rng, nt, box=(0.0, 640.0, 0.0, 480.0)):
    t_xy = np.stack([rng.uniform(box[0], box[1], nt), rng.uniform(box[2], box[3], nt)], 1).astype(np.float32)
    return t_xy, rng.integers(2, 5, nt).astype(np.int32), rng.integers(0, 256, (nt, 32), dtype=np.uint8)


def _near(rng, desc, bits=4):
    d = desc.copy()
    for b in rng.integers(0, 256, (bits, len(d))):
        d[np.arange(len(d)), b // 8] ^= (1 << (b % 8)).astype(np.uint8)
    return d


def _window_counts(q_xy, margin, t_xy, valid):
    """Keypoints within `margin` of each valid query in x and in y: what get_keypoints_in_cell lists when every level is admitted."""
    n = 0
    for q in np.flatnonzero(valid):
        n += int(((np.abs(t_xy[:, 0] - q_xy[q, 0]) <= margin) & (np.abs(t_xy[:, 1] - q_xy[q, 1]) <= margin)).sum())
    return n


def _cell_problem(nq, nt, margin, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    t_xy, t_oct, td = _keypoints(rng, nt)
    pick = rng.integers(0, nt, nq)
    q_xy = (t_xy[pick] + rng.normal(0, 1.0, (nq, 2)) + shift).astype(np.float32)
    return dict(qd=_near(rng, td[pick]), q_xy=q_xy, q_margin=np.full(nq, margin, np.float32), td=td, t_xy=t_xy, t_oct=t_oct,
                q_valid=(rng.uniform(size=nq) < 0.9).astype(np.uint8), occupied=(rng.uniform(size=nt) < 0.05).astype(np.uint8))


def _in_cells(ctx, p):
    from stella_vslam_amd import match
    out, num = match.projection(0.8, False, ctx).match_in_cells(p["qd"], p["q_xy"], p["q_margin"], p["td"], p["t_xy"], p["t_oct"], BOUNDS,
                                                                match.MATCH_RATIO_SAME_OCTAVE, 100, q_valid=p["q_valid"], occupied=p["occupied"])
    return out, np.array(num)


def _in_cells_oracle(p):
    from oracle import oracle as O
    x, y = p["t_xy"][:, 0].copy(), p["t_xy"][:, 1].copy()
    off_g, items = O.assign_keypoints_to_grid(x, y, BOUNDS)
    cand_off, cand_idx = [0], []
    for q in range(len(p["qd"])):
        if p["q_valid"][q]:
            cand_idx += O.get_keypoints_in_cell(x, y, p["t_oct"], off_g, items, BOUNDS, float(p["q_xy"][q, 0]), float(p["q_xy"][q, 1]),
                                                float(p["q_margin"][q])).tolist()
        cand_off.append(len(cand_idx))
    exp = O.match_candidates(p["qd"], p["td"], cand_off, cand_idx, check_orientation=False, thr=100, lowe_ratio=0.8, mode=1, t_octave=p["t_oct"],
                             q_valid=p["q_valid"], occupied=p["occupied"])
    return exp, len(cand_idx)


GRANULE_LISTS = 131072  # candidates of 8 bytes that fill the 1 MiB scratch granule


def test_match_in_cells_small_large_small():
    small, large = _cell_problem(3, 5, 20.0, 0), _cell_problem(2000, 20000, 20.0, 1)
    exp, total = _in_cells_oracle(large)
    assert total > GRANULE_LISTS  # on the shared context: a guess from the small call that falls short, and lists that make the arena regrow
    _same_on_fresh_contexts(_in_cells, [small, large, small, large])  # (the last: a guess that suffices, against the exact sizing)
    got, num = _in_cells(_context(), large)
    assert np.array_equal(got, exp) and num == (exp >= 0).sum() > 1000


def test_match_in_cells_guess_falls_short_without_regrowth():
    """The reuse path: the second pass finds the arena of the first as it left it.  A sparse call leaves a guess of little more than 4 096
    candidates and a 1 MiB arena; the dense call that follows overruns the guess and still fits 1 MiB with its lists (some 150 KB of
    keypoints, queries and state, 80 KB of lists).  No entry point reports the arena's size, so that it did not grow is argued here, not
    asserted; the result is asserted, against the exact sizing of a fresh context and against the oracle."""
    sparse, dense = _cell_problem(50, 2000, 5.0, 2), _cell_problem(500, 2000, 28.0, 3)
    exp, total = _in_cells_oracle(dense)
    assert _in_cells_oracle(sparse)[1] < 1000 and 4096 + 1250 < total < 20000
    _same_on_fresh_contexts(_in_cells, [sparse, dense])
    got, num = _in_cells(_context(), dense)
    assert np.array_equal(got, exp) and num == (exp >= 0).sum() > 100


def _landmark_problem(n, nt, margin, seed, box=(0.0, 640.0, 0.0, 480.0), stereo=False):
    """Landmarks on the rays of `n` keypoints, seen from the identity pose at level 3 (window = margin x 1.2^3)."""
    rng = np.random.default_rng(seed)
    t_xy, t_oct, td = _keypoints(rng, nt, box)
    pick = rng.integers(0, nt, n)
    target = t_xy[pick] if box[1] > 600.0 else np.stack([rng.uniform(300, 600, n), rng.uniform(100, 400, n)], 1)  # (a corner box: landmarks elsewhere)
    depth = rng.uniform(2.0, 9.0, n)
    pw = np.stack([(target[:, 0] - CX) / FX * depth, (target[:, 1] - CY) / FX * depth, depth], 1)
    dist = np.linalg.norm(pw, axis=1)
    mx = (dist * 1.2 ** 2.5).astype(np.float32)
    xr = None
    if stereo:
        xr = np.where(rng.uniform(size=nt) < 0.5, t_xy[:, 0] - rng.uniform(2, 20, nt), -1.0).astype(np.float32)
    return dict(pw=pw, nv=pw / dist[:, None], mn=(mx / np.float32(1.2 ** 7) * np.float32(0.5)).astype(np.float32), mx=mx, lm_desc=_near(rng, td[pick]),
                skip=(rng.uniform(size=n) < 0.1).astype(np.uint8), occupied=(rng.uniform(size=nt) < 0.05).astype(np.uint8), td=td, t_xy=t_xy, t_oct=t_oct,
                t_xright=xr, margin=margin)


def _camera(ctx, stereo=False):
    from stella_vslam_amd import camera
    return camera.perspective("c", "Stereo" if stereo else "Monocular", "Gray", 640, 480, 30.0, FX, FX, CX, CY, 0.0, 0.0, 0.0, 0.0, 0.0,
                              focal_x_baseline=40.0 if stereo else 0.0, ctx=ctx)


SF = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
LSF = float(np.log(np.float32(1.2)))
EYE, ZERO = np.eye(3), np.zeros(3)


def _frame_and_landmarks(ctx, p, bound=False):
    from stella_vslam_amd import data, match
    from stella_vslam_amd.feature import KEYPOINT_DTYPE
    k = np.zeros(len(p["t_xy"]), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = p["t_xy"][:, 0], p["t_xy"][:, 1], p["t_oct"]
    cam = _camera(ctx)
    obs = types.SimpleNamespace(descriptors_=p["td"], undist_keypts_=k, stereo_x_right_=None, num_grid_cols_=64, num_grid_rows_=48)
    if bound:  # the keypoint side from a resident frame: the arrays passed beside it are garbage
        rf = data.resident_frame(ctx).upload(cam, k, p["td"])
        rf.bind()
        obs = types.SimpleNamespace(descriptors_=np.zeros_like(p["td"]), undist_keypts_=np.zeros_like(k), stereo_x_right_=None, num_grid_cols_=3,
                                    num_grid_rows_=3)
    out, num, vis, rp, xr, lv = match.projection(0.8, False, ctx).match_frame_and_landmarks(
        cam, EYE, ZERO, p["pw"], p["nv"], p["mn"], p["mx"], p["lm_desc"], obs, SF, LSF, margin=p["margin"], skip=p["skip"], occupied=p["occupied"])
    return out, np.array(num), vis, rp, xr, lv


def _visible_windows(ctx, p):
    vis, rp, _, lv = _camera(ctx).reproject_landmarks(EYE, ZERO, p["pw"], p["nv"], p["mn"], p["mx"], 0.5, 8, LSF, skip=p["skip"])
    assert (lv[vis == 1] == 3).all()
    return _window_counts(rp, float(np.float32(p["margin"]) * SF[3]), p["t_xy"], vis == 1)


def test_match_frame_and_landmarks_small_large_small():
    """All four observability outputs are asked for and compared with the matches."""
    small, large = _landmark_problem(3, 5, 12.0, 0), _landmark_problem(2000, 20000, 12.0, 1)
    assert _visible_windows(_context(), large) > GRANULE_LISTS
    _same_on_fresh_contexts(_frame_and_landmarks, [small, large, small])
    out, num, vis, _, _, _ = _frame_and_landmarks(_context(), large)
    assert num == (out >= 0).sum() > 1000 and 1500 < vis.sum() < 2000 and (out[vis == 0] == -1).all()


def test_match_frame_and_landmarks_on_a_bound_frame_small_large_small():
    small, large = _landmark_problem(3, 5, 12.0, 2), _landmark_problem(2000, 20000, 12.0, 3)
    shared = _context()
    for k, p in enumerate([small, large, small]):
        got, exp = _frame_and_landmarks(shared, p, bound=True), _frame_and_landmarks(_context(), p)
        for g, e in zip(got, exp):
            assert g.tobytes() == e.tobytes(), f"call {k}"


def _fuse(ctx, p):
    from stella_vslam_amd import match
    out, num = match.fuse(0.6, ctx).detect_duplication(_camera(ctx, True), EYE, ZERO, p["pw"], 1 - p["skip"], p["mn"], p["mx"], p["nv"], p["lm_desc"], SF,
                                                       (1.0 / (SF * SF)).astype(np.float32), LSF, p["margin"], p["td"], p["t_xy"], p["t_oct"],
                                                       t_xright=p["t_xright"], do_reprojection_matching=True)
    return out, np.array(num)


def test_fuse_detect_duplication_small_large_small():
    """The chi-square gate on the reprojection (fuse.cc:92-119) with stereo keypoints: gated per candidate, the lists are as long without it."""
    small, large = _landmark_problem(3, 5, 12.0, 4, stereo=True), _landmark_problem(2000, 20000, 12.0, 5, stereo=True)
    assert _visible_windows(_context(), large) > GRANULE_LISTS
    _same_on_fresh_contexts(_fuse, [small, large, small])
    assert _fuse(_context(), large)[1] > 300


def _bucket_problem(n, seed, nodes=8):
    """Every descriptor within 8 bits of one base, so that no pair of a bucket fails a Hamming cut-off: the lists are the buckets."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    side = lambda: dict(desc=_near(rng, np.repeat(base, n, 0)), angle=rng.uniform(0, 360, n).astype(np.float32), node=rng.integers(0, nodes, n).astype(np.int32),
                        valid=(rng.uniform(size=n) < 0.9).astype(np.uint8), bearings=(lambda b: b / np.linalg.norm(b, axis=1, keepdims=True))(rng.normal(size=(n, 3))))
    a, b = side(), side()
    total = int(np.bincount(b["node"][b["valid"] == 1], minlength=nodes)[a["node"][a["valid"] == 1]].sum())
    return a, b, (rng.uniform(size=n) < 0.05).astype(np.uint8), rng.integers(0, 8, n).astype(np.int32), total


def _bow(ctx, p):
    from stella_vslam_amd import match
    a, b, occ, _, _ = p
    out, num = match.bow_tree(0.9, False, ctx).match(a["desc"], a["angle"], a["valid"], a["node"], b["desc"], b["angle"], b["node"], valid2=b["valid"],
                                                     occupied2=occ)
    return out, np.array(num)


def _triangulation_kw(p):
    a, b, _, octave, _ = p
    return dict(desc1=a["desc"], angle1=a["angle"], octave1=octave, bearings1=a["bearings"], has_lm1=1 - a["valid"], desc2=b["desc"], angle2=b["angle"],
                bearings2=b["bearings"], has_lm2=1 - b["valid"], E_12=np.array([[0.0, -0.1, 0.2], [0.1, 0.0, -0.3], [-0.2, 0.3, 0.0]]),
                epipole_in_2=np.array([0.0, 0.0, 1.0]), valid_epipole=0, scale_factors=SF, residual_rad_thr=10.0, node1=a["node"], node2=b["node"])


def _triangulation(ctx, p):
    from stella_vslam_amd import match
    out, num = match.match_for_triangulation(ctx, 0.9, False, **_triangulation_kw(p))
    return out, np.array(num)


def test_bow_match_small_large_small():
    from oracle import oracle as O
    small, large = _bucket_problem(3, 0, nodes=1), _bucket_problem(2000, 1)
    assert large[4] > GRANULE_LISTS
    _same_on_fresh_contexts(_bow, [small, large, small])
    a, b, occ, _, _ = large
    exp, _ = O.bow_match(0.9, False, a["desc"], a["angle"], a["valid"], a["node"], b["desc"], b["angle"], b["node"], valid2=b["valid"], occupied2=occ)
    got, num = _bow(_context(), large)
    assert np.array_equal(got, exp) and num == (exp >= 0).sum() > 100


def test_match_for_triangulation_small_large_small():
    """No epipole, a residual threshold no pair fails: every valid pair of a bucket is a candidate."""
    from oracle import oracle as O
    small, large = _bucket_problem(3, 2, nodes=1), _bucket_problem(2000, 3)
    assert large[4] > GRANULE_LISTS
    _same_on_fresh_contexts(_triangulation, [small, large, small])
    exp, _ = O.match_for_triangulation(0.9, False, **_triangulation_kw(large))
    got, num = _triangulation(_context(), large)
    assert np.array_equal(got, exp) and num == (exp >= 0).sum() > 100


def test_two_pass_matchers_without_a_candidate():
    """Queries whose windows hold no keypoint, sized exactly (a fresh context) and by a guess (a context that has matched before): every match
    is -1, the count 0, and svgpu_match_frame_and_landmarks still returns what the reprojection found."""
    warm, dense = _context(), _cell_problem(500, 2000, 28.0, 3)
    assert _in_cells(warm, dense)[1] > 100
    empty = _cell_problem(300, 2000, 20.0, 6, shift=5000.0)
    lms = _landmark_problem(300, 2000, 12.0, 7, box=(0.0, 100.0, 0.0, 60.0))  # keypoints in one corner, landmarks elsewhere
    assert _visible_windows(_context(), lms) == 0
    vis, rp, xr, lv = _camera(_context()).reproject_landmarks(EYE, ZERO, lms["pw"], lms["nv"], lms["mn"], lms["mx"], 0.5, 8, LSF, skip=lms["skip"])
    assert 200 < vis.sum() < 300
    for ctx in (_context(), warm):
        out, num = _in_cells(ctx, empty)
        assert num == 0 and (out == -1).all()
        out, num, *obs = _frame_and_landmarks(ctx, lms)
        assert num == 0 and (out == -1).all()
        for g, e in zip(obs, (vis, rp, xr, lv)):
            assert g.tobytes() == e.tobytes()
        assert _in_cells(ctx, dense)[1] > 100  # (and the context goes on matching)
