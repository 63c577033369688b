"""GPU: the hand-written device scan and stable radix sort (csrc/sv_sort.hip) against numpy, at sizes either side of every tile boundary
(one-workgroup scan <= 16384 elements, many-workgroup scan in tiles of 4096, radix tiles of 2048); below them the radix sort on every key
class and with a device-side count, the one-workgroup sorts (one side, several sides in one launch) and the bucket order on either side
of the small-sort limit.  Integer work throughout: the bar is equality with numpy."""
import ctypes as C
import numpy as np
import pytest

from tests import sort_problems as SP

pytestmark = pytest.mark.gpu


def _run(ctx, L, values=None, keys=None, bits=32):
    n = len(values if values is not None else keys)
    scan = np.zeros(n + 1, np.int32) if values is not None else None
    idx = np.zeros(max(n, 1), np.int32) if keys is not None else None
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = L.svgpu_selftest_scan_sort(ctx.handle, n, p(values), p(scan), p(keys), bits, p(idx))
    ctx.check(rc, "svgpu_selftest_scan_sort")
    return scan, idx


@pytest.mark.parametrize("n", [0, 1, 63, 64, 1000, 4095, 4096, 4097, 16383, 16384, 16385, 20480, 65537, 200001, 1 << 20])
def test_scan_matches_numpy(n):
    from stella_vslam_amd import feature
    from stella_vslam_amd._lib import lib
    rng = np.random.default_rng(n)
    v = rng.integers(0, 30, n).astype(np.int32)
    scan, _ = _run(feature.Context(0), lib(), values=v)
    ref = np.concatenate([[0], np.cumsum(v, dtype=np.int64)]).astype(np.int32)
    assert np.array_equal(scan, ref)


@pytest.mark.parametrize("n,bits", [(1, 1), (2047, 6), (2048, 7), (2049, 12), (50000, 17), (300000, 18), (1 << 20, 32)])
def test_radix_sort_is_stable(n, bits):
    from stella_vslam_amd import feature
    from stella_vslam_amd._lib import lib
    rng = np.random.default_rng(n + bits)
    k = rng.integers(0, min(1 << bits, 1 << 31), n, dtype=np.int64).astype(np.uint32)
    _, idx = _run(feature.Context(0), lib(), keys=k, bits=bits)
    ref = np.argsort(k, kind="stable").astype(np.int32)
    assert np.array_equal(idx[:n], ref)


def _scan_one_launch(gpu, values):
    ctx, L = gpu
    scan = np.full(len(values) + 1, -7, np.int32)
    rc = L.svgpu_selftest_scan_one_launch(ctx.handle, len(values), C.c_void_p(values.ctypes.data), C.c_void_p(scan.ctypes.data))
    ctx.check(rc, "svgpu_selftest_scan_one_launch")
    return scan


@pytest.mark.parametrize("n", [0, 1, 16383, 16384, 16385, 32767, 32768, 32769, 50000])
def test_scan_without_scratch_walks_its_tiles(gpu, n):
    """sv_scan_i32 without scratch (the grid and bucket lists' form): one workgroup over tiles of 16 384 elements -- either side of the first
    and the second tile boundary, a last tile that is not full; the total behind the data."""
    v = np.random.default_rng(n).integers(0, 30, n).astype(np.int32)
    scan = _scan_one_launch(gpu, v)
    assert np.array_equal(scan, np.concatenate([[0], np.cumsum(v, dtype=np.int64)]).astype(np.int32))
    assert scan[n] == v.sum()


def test_scan_without_scratch_of_zeros_over_three_tiles(gpu):
    scan = _scan_one_launch(gpu, np.zeros(32769, np.int32))
    assert scan.shape == (32770,) and not scan.any()


# ---- the paths the two tests above do not reach (tests/sort_problems.py: key classes, sizes and the numpy references; its CPU test shows that
# the classes tell an unstable sort, a sort by the full key and a sort that ignores the device count from the right one)
RADIX_COUNT, SMALL, SIDES, BUCKET = 0, 1, 2, 3  # SVGPU_SORT_PATH_* of include/svgpu.h


@pytest.fixture(scope="module")
def gpu():
    from stella_vslam_amd import feature
    from stella_vslam_amd._lib import lib
    return feature.Context(0), lib()


def _paths(gpu, path, n, total, count=0, start=0, bits=32, keys=None, idx=None, node=None, sides=None):
    """svgpu_selftest_sort_paths: (keys_out, idx_out, info) with `total` output elements"""
    ctx, L = gpu
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    ko, io, info = np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.int32), np.full(4, -7, np.int32)
    rc = L.svgpu_selftest_sort_paths(ctx.handle, path, n, count, start, bits, p(keys), p(idx), p(node), p(sides), p(ko), p(io), p(info))
    ctx.check(rc, "svgpu_selftest_sort_paths")
    return ko[:total], io[:total], info


def test_scan_of_zeros_beyond_one_workgroup(gpu):
    scan, _ = _run(gpu[0], gpu[1], values=np.zeros(16385, np.int32))
    assert scan.shape == (16386,) and not scan.any()


@pytest.mark.parametrize("n", SP.RADIX_N)
@pytest.mark.parametrize("name", SP.KEY_CLASSES)
def test_radix_key_classes_host_count(gpu, name, n):
    """Every key class at every `bits` it applies to: stable, by the low `bits` key bits only."""
    for bits in SP.RADIX_BITS:
        if SP.applies(name, bits):
            k = SP.keys(name, n, bits)
            _, idx = _run(gpu[0], gpu[1], keys=k, bits=bits)
            assert np.array_equal(idx[:n], SP.radix_order(k, bits)), bits


@pytest.mark.parametrize("n", SP.RADIX_SCAN_SWITCH)
@pytest.mark.parametrize("name", ["uniform", "runs"])
def test_radix_where_the_histogram_scan_switches_kernels(gpu, name, n):
    """64 bins x 256 tiles = 16 384 histogram entries take the one-workgroup scan, 64 x 257 the tiled one."""
    k = SP.keys(name, n, 13)
    _, idx = _run(gpu[0], gpu[1], keys=k, bits=13)
    assert np.array_equal(idx[:n], SP.radix_order(k, 13))


@pytest.mark.parametrize("n", SP.COUNT_N)
def test_radix_device_count(gpu, n):
    """The launches are sized for n, the count is read on the device (every local BA): the first `count` results are the stable order of the
    first `count` pairs, whichever buffer set the data starts in; stale smallest keys lie behind the count."""
    rng = np.random.default_rng(n)
    vals = rng.permutation(n).astype(np.int32)
    for count in SP.counts(n):
        for start in (0, 1):
            for bits in SP.COUNT_BITS:
                for name in ("high_bits", "runs"):
                    k = SP.counted(name, n, count, bits)
                    ko, io, info = _paths(gpu, RADIX_COUNT, n, count, count=count, start=start, bits=bits, keys=k, idx=vals)
                    o = SP.radix_order(k, bits, count)
                    what = (count, start, bits, name)
                    assert info[0] == start ^ (-(-bits // 6) & 1), what       # the documented return value: start ^ (passes & 1)
                    assert info[1] == 1, what                                 # 64-bit values moved whole
                    assert np.array_equal(ko, k[o]) and np.array_equal(io, vals[o]), what


@pytest.mark.parametrize("n", SP.SMALL_N)
def test_sort_small(gpu, n):
    """The one-workgroup bitonic network on (key, index) composites: duplicate-heavy keys with 0xFFFFFFFF among them, indices a random
    permutation.  The device must grant the LDS at every size (4 097 and up need more than 48 KB)."""
    rng = np.random.default_rng(n)
    idx = rng.permutation(n).astype(np.int32)
    for name in SP.SMALL_CLASSES:
        for k in (SP.keys(name, n, 32), SP.with_max(SP.keys(name, n, 32))):
            ko, io, info = _paths(gpu, SMALL, n, n, keys=k, idx=idx)
            o = SP.small_order(k, idx)
            assert info[0] == 1, name
            assert np.array_equal(ko, k[o]) and np.array_equal(io, idx[o]), name


def _sides_problem(sizes, no_node=(), seed=0):
    """(table, concatenated node ids, [(node | None, n)]) -- about a fifth of a side's keypoints without a node (negative ids, not only -1)"""
    rng = np.random.default_rng(seed)
    tab, cat, per = [], [], []
    for u, m in enumerate(sizes):
        node = SP.nodes(m, distinct=max(m // 5, 1), negative=0.0, seed=u)
        neg = rng.uniform(0, 1, m) < 0.2
        node[neg] = -rng.integers(1, 1 << 31, int(neg.sum()))
        tab += [m, 0 if u in no_node else 1]
        cat.append(node)
        per.append((None if u in no_node else node, m))
    return np.array(tab, np.int32), np.concatenate(cat).astype(np.int32), per


def test_sort_small_sides_in_one_launch(gpu):
    sizes = SP.SIDES_N + [300, 16384]
    no_node = (2, 4, len(sizes) - 1)  # sides of 64, 1 025 and 16 384 keypoints without node ids: identity order
    tab, cat, per = _sides_problem(sizes, no_node)
    total = int(sum(sizes))
    ko, io, info = _paths(gpu, SIDES, len(sizes), total, node=cat, sides=tab)
    assert info[0] == 1 and info[1] == SP.SMALL_MAX
    first = 0
    for u, (node, m) in enumerate(per):
        gk, gi = ko[first:first + m], io[first:first + m]
        if m > SP.SMALL_MAX:  # left to the general sort: not written
            assert (gk == SP.SENTINEL).all() and (gi.view(np.uint32) == SP.SENTINEL).all(), u
        else:
            ek, ei = SP.side_order(node, m)
            assert np.array_equal(gk, ek) and np.array_equal(gi, ei), (u, m)
            assert node is None or m < 64 or ((ek == 0xFFFFFFFF).any() and (ek != 0xFFFFFFFF).any())
        first += m
    # nothing for the launch to do: every side is empty or beyond the limit (max_n = 0)
    sizes = [SP.SMALL_MAX + 1, 0, 20000, 0]
    tab, cat, per = _sides_problem(sizes)
    ko, io, info = _paths(gpu, SIDES, len(sizes), int(sum(sizes)), node=cat, sides=tab)
    assert info[0] == 1 and info[1] == 0
    assert (ko == SP.SENTINEL).all() and (io.view(np.uint32) == SP.SENTINEL).all()


@pytest.mark.parametrize("n,with_nodes", [(m, True) for m in SP.BUCKET_N] + [(SP.SMALL_MAX + 1, False)])
def test_bucket_sort_both_sides_of_the_small_sort_limit(gpu, n, with_nodes):
    """sv_bucket_sort: the one-workgroup sort up to 16 384 keypoints, beyond it the radix sort on widened values -- the same numpy
    reference on both sides of the switch; about 4 000 distinct node ids and 5 % keypoints without one."""
    node = SP.nodes(n) if with_nodes else None
    ko, io, info = _paths(gpu, BUCKET, n, n, node=node)
    ek, ei = SP.side_order(node, n)
    assert info[0] == (1 if n > SP.SMALL_MAX else 0)
    assert np.array_equal(ko, ek) and np.array_equal(io, ei)
