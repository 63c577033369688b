"""GPU parity of the brute-force matcher (k_bf_binsort -> k_bf_mfma | k_bf_topk -> k_bf_replay) on its boundaries: every planted class of
tests/bf_problems.py through svgpu_match_bruteforce, the sizes where tiles, blocks, replay shapes, register caches and owner tables
change, and the batched device entry points with empty / over-full pairs, poisoned padding and valid2 masks.  Lists and counts must
equal O.brute_force_match.  The whole module runs once more in a fresh process with SVGPU_BF_VALU=1 (the VALU distance kernel)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import bf_problems as BP

pytestmark = pytest.mark.gpu

CLASSES = ["threshold", "ratio_equality", "around_dmax", "ties", "popcount", "orientation", "domino", "valid2"]


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd import feature
    return feature.Context()


@pytest.fixture(scope="module")
def classes():
    return BP.all_classes(big=True)


def _gpu(ctx, d1, a1, d2, a2, valid2, ratio, check):
    from stella_vslam_amd import match
    pairs, out = match.robust(ratio, check, ctx).brute_force_match(d1, a1, d2, a2, valid2)
    return out, len(pairs)


@pytest.mark.parametrize("cls", CLASSES)
def test_planted_class_matches_oracle(ctx, classes, cls):
    bad = []
    for case in classes[cls]:
        out, num = _gpu(ctx, *case.args(), case.ratio, case.check)
        exp = case.oracle()
        if not (np.array_equal(out, exp) and num == (exp >= 0).sum()):
            bad.append((case.name, int((out != exp).sum())))
    assert not bad, bad


@pytest.mark.parametrize("check", [0, 1])
@pytest.mark.parametrize("qa", [float("nan"), -600.0, -1000.0, -500.0])
def test_query_angle_is_never_a_liveness_marker(ctx, qa, check):
    """Live queries whose angle is NaN or <= -500 match as the reference does (ignored angles with check_orientation 0; a NaN difference is
    never gated, equal angles never are) -- on the MFMA path (lowe_ratio 0.75) as on every other."""
    rng = np.random.default_rng(17)
    n1, n2 = 700, 600
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    src = rng.permutation(n1)[:n2]
    d2 = np.stack([BP.at_distance(rng, d1[s], int(rng.integers(0, 30))) for s in src])
    a1 = np.full(n1, np.float32(qa), np.float32)
    a2 = np.full(n2, np.float32(qa), np.float32)
    a2[::3] = 12.0   # some ordinary queries beside them
    a1[src[::3]] = 20.0
    exp = O.brute_force_match(d1, a1, d2, a2, None, 0.75, bool(check))
    assert (exp >= 0).sum() > n2 // 2
    out, num = _gpu(ctx, d1, a1, d2, a2, None, 0.75, bool(check))
    assert np.array_equal(out, exp) and num == (exp >= 0).sum()


def _random_planted(seed, n1, n2):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    src = rng.integers(0, n1, n2)
    src[: min(n2, 8)] = np.arange(n1 - 1, max(n1 - 9, -1), -1)[: min(n2, 8)]  # the highest side-1 indices are planted matches
    flips = rng.integers(0, 46, n2)
    mask = rng.random((n2, 256)).argsort(1).argsort(1) < flips[:, None]  # exactly flips[j] random bits of row j
    d2 = d1[src] ^ np.packbits(mask, axis=1, bitorder="little")
    if n2 > 4:
        d2[3] = d1[src[2]]            # exact copies, and a duplicated target
        d1[(src[2] + 1) % n1] = d1[src[2]]
    a1 = rng.uniform(0, 360, n1).astype(np.float32)
    a2 = ((a1[src] + rng.normal(0, 12, n2)) % 360).astype(np.float32)
    valid2 = (rng.uniform(size=n2) < 0.9).astype(np.uint8)
    return d1, a1, d2, a2, valid2


# (n1, n2): 1 (no second candidate) / the 32-target MFMA tile / the 256-query block and 256-target chunk / the k_bf_replay<5,512> vs
# <4,1024> switch at 2 560 / the register-cached rows up to 4 096 / owner tables in LDS up to cap1 + cap2 = 24 576, global beyond /
# 65 535 targets (the largest index the 16-bit packed keys carry)
SIZES = [(1, 1), (1, 40), (40, 1), (31, 31), (32, 32), (33, 33), (31, 33), (255, 256), (256, 257), (257, 255), (2560, 2560), (2561, 2561),
         (4096, 4096), (4097, 4097), (12288, 12288), (12289, 12288), (65535, 300)]


@pytest.mark.parametrize("n1,n2", SIZES)
def test_sizes_match_oracle(ctx, n1, n2):
    d1, a1, d2, a2, valid2 = _random_planted(n1 * 7 + n2, n1, n2)
    for ratio, check, v in ((0.75, True, None), (0.8, False, valid2)):
        exp = O.brute_force_match(d1, a1, d2, a2, v, ratio, check)
        if min(n1, n2) >= 30:
            assert (exp >= 0).sum() > min(n1, n2) // 4
        out, num = _gpu(ctx, d1, a1, d2, a2, v, ratio, check)
        assert np.array_equal(out, exp) and num == (exp >= 0).sum(), (ratio, check, int((out != exp).sum()))


def _records(angles):
    rec = np.zeros(len(angles), O.KEYPOINT_DTYPE)
    rec["angle"] = angles
    return rec


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("ratio,check", [(0.8, 1), (0.75, 0), (0.3, 1)])
def test_batch_device_pairs_with_empty_full_and_clamped_counts(ctx, ratio, check):
    """svgpu_match_bruteforce_batch_device: per-pair counts below cap, zero on either side, above cap (clamped to cap), n_stride 3, a
    valid2 mask.  Every slot beyond a pair's count holds poison -- exact copies of the live descriptors of the other side, NaN angles -- and
    is never matched; matched_dev starts as -7 and rows [n1, cap1) come back -1."""
    import torch
    from stella_vslam_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(23)
    P, cap1, cap2, ns = 6, 320, 288, 3
    n1 = [320, 0, 150, 401, 77, 200]
    n2 = [288, 100, 0, 500, 288, 1]
    D1 = np.zeros((P, cap1, 32), np.uint8)
    D2 = np.zeros((P, cap2, 32), np.uint8)
    A1 = np.zeros((P, cap1), np.float32)
    A2 = np.zeros((P, cap2), np.float32)
    V2 = (rng.uniform(size=(P, cap2)) < 0.85).astype(np.uint8)
    for p in range(P):
        c1, c2 = min(n1[p], cap1), min(n2[p], cap2)
        D1[p] = rng.integers(0, 256, (cap1, 32), dtype=np.uint8)
        A1[p] = rng.uniform(0, 360, cap1)
        src = rng.integers(0, max(c1, 1), cap2)
        D2[p] = np.stack([BP.at_distance(rng, D1[p, s], int(rng.integers(0, 30))) for s in src])
        A2[p] = (A1[p, src] + rng.normal(0, 10, cap2)) % 360
        if c1 < cap1 and c2 > 0:     # poison: side-1 padding = copies of the live queries
            D1[p, c1:] = D2[p, rng.integers(0, c2, cap1 - c1)]
            A1[p, c1:] = np.nan
        if c2 < cap2 and c1 > 0:     # side-2 padding = copies of the live targets
            D2[p, c2:] = D1[p, rng.integers(0, c1, cap2 - c2)]
            A2[p, c2:] = np.nan
            V2[p, c2:] = 1
    cnt1 = np.full(P * ns, 999999, np.int32)
    cnt2 = np.full(P * ns, 999999, np.int32)
    cnt1[::ns], cnt2[::ns] = n1, n2
    t = dict(d1=_dev(D1.reshape(-1)), d2=_dev(D2.reshape(-1)), k1=_dev(_records(A1.reshape(-1)).view(np.uint8)),
             k2=_dev(_records(A2.reshape(-1)).view(np.uint8)), c1=_dev(cnt1), c2=_dev(cnt2), v2=_dev(V2.reshape(-1)))
    matched = torch.full((P * cap1,), -7, dtype=torch.int32, device="cuda")
    num = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(L.svgpu_match_bruteforce_batch_device(ctx.handle, P, _ptr(t["d1"]), _ptr(t["k1"]), _ptr(t["c1"]), cap1, _ptr(t["d2"]), _ptr(t["k2"]),
                                                    _ptr(t["c2"]), cap2, ns, _ptr(t["v2"]), C.c_float(ratio), check, _ptr(matched), _ptr(num), None),
              "batch")
    ctx.synchronize()
    got, gnum = matched.cpu().numpy().reshape(P, cap1), num.cpu().numpy()
    total = 0
    for p in range(P):
        c1, c2 = min(n1[p], cap1), min(n2[p], cap2)
        exp = O.brute_force_match(D1[p, :c1], A1[p, :c1], D2[p, :c2], A2[p, :c2], V2[p, :c2], ratio, bool(check))
        assert np.array_equal(got[p, :c1], exp) and (got[p, c1:] == -1).all() and gnum[p] == (exp >= 0).sum(), p
        total += gnum[p]
    assert total > 300


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("ratio,check", [(0.8, 1), (0.3, 0)])
def test_consecutive_ring_with_empty_and_clamped_frames(ctx, packed, ratio, check):
    """svgpu_match_consecutive_batch_device (records) and _angles (packed angles), ring mode with one sorted copy per frame: pair t = frame
    (t + 1) % F against frame t, frames with zero and with more than cap keypoints, a valid mask, poisoned padding (copies of the live
    descriptors of both neighbours, NaN angles)."""
    import torch
    from stella_vslam_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(29)
    F, cap, ns = 5, 300, 2
    n = [300, 0, 180, 450, 120]
    c = [min(x, cap) for x in n]
    D = np.zeros((F, cap, 32), np.uint8)
    A = np.zeros((F, cap), np.float32)
    D[0] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    A[0] = rng.uniform(0, 360, cap)
    for f in range(1, F):  # frame f: noisy copies of frame f - 1 (and fresh descriptors where that frame had none)
        src = rng.integers(0, cap, cap)
        D[f] = np.stack([BP.at_distance(rng, D[f - 1, s], int(rng.integers(0, 30))) for s in src])
        A[f] = (A[f - 1, src] + rng.normal(0, 10, cap)) % 360
    for f in range(F):
        nb = [g for g in ((f - 1) % F, (f + 1) % F) if c[g] > 0]
        for k in range(c[f], cap):
            g = nb[k % len(nb)]
            D[f, k] = D[g, rng.integers(0, c[g])]
            A[f, k] = np.nan
    V = (rng.uniform(size=(F, cap)) < 0.85).astype(np.uint8)
    cnt = np.full(F * ns, 999999, np.int32)
    cnt[::ns] = n
    td, tk, tc, tv = _dev(D.reshape(-1)), _dev(_records(A.reshape(-1)).view(np.uint8)), _dev(cnt), _dev(V.reshape(-1))
    matched = torch.full((F * cap,), -7, dtype=torch.int32, device="cuda")
    num = torch.full((F,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if packed:
        ta = _dev(A.reshape(-1))
        ctx.check(L.svgpu_match_consecutive_batch_device_angles(ctx.handle, F, _ptr(td), _ptr(tk), _ptr(ta), _ptr(tc), cap, ns, _ptr(tv), C.c_float(ratio),
                                                                check, _ptr(matched), _ptr(num), None), "ring, packed angles")
    else:
        ctx.check(L.svgpu_match_consecutive_batch_device(ctx.handle, F, _ptr(td), _ptr(tk), _ptr(tc), cap, ns, _ptr(tv), C.c_float(ratio), check,
                                                         _ptr(matched), _ptr(num), None), "ring")
    ctx.synchronize()
    got, gnum = matched.cpu().numpy().reshape(F, cap), num.cpu().numpy()
    total = 0
    for t in range(F):
        f = (t + 1) % F
        exp = O.brute_force_match(D[f, :c[f]], A[f, :c[f]], D[t, :c[t]], A[t, :c[t]], V[t, :c[t]], ratio, bool(check))
        assert np.array_equal(got[t, :c[f]], exp) and (got[t, c[f]:] == -1).all() and gnum[t] == (exp >= 0).sum(), t
        total += gnum[t]
    assert total > (200 if ratio > 0.5 else 80)


def test_whole_module_again_with_the_valu_distance_kernel():
    """SVGPU_BF_VALU is read once per process: the module once more in a fresh one, every list from k_bf_topk instead of k_bf_mfma."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SVGPU_BF_VALU="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "tests/test_gpu_bf_edges.py", "-k", "not valu_distance_kernel"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
