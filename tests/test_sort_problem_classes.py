"""The key classes of tests/sort_problems.py are what they claim, the references agree with a literal restatement of each sort, and three
deliberately wrong sorts -- unstable, ordering by the full key, ignoring the device count -- are told from the right one by every class
meant to expose them (so the GPU tests built on these classes can catch those faults).  No GPU."""
import pathlib

import numpy as np
import pytest

from tests import sort_problems as SP

ROOT = pathlib.Path(__file__).resolve().parent.parent
ALL_N = sorted(set(SP.RADIX_N + SP.RADIX_SCAN_SWITCH + SP.COUNT_N))


def _runs(k):
    """lengths of the maximal runs of equal keys"""
    cut = np.flatnonzero(np.diff(k.astype(np.int64)) != 0) + 1
    return np.diff(np.concatenate([[0], cut, [len(k)]]))


@pytest.mark.parametrize("name", SP.KEY_CLASSES)
def test_classes_are_what_they_claim(name):
    for n in ALL_N:
        for bits in SP.RADIX_BITS:
            if not SP.applies(name, bits):
                continue
            k = SP.keys(name, n, bits)
            m = SP.mask(bits)
            assert k.dtype == np.uint32 and k.shape == (n,) and np.array_equal(k, SP.keys(name, n, bits)), (n, bits)
            if name not in ("high_bits", "top_digit"):
                assert not (k & ~m).any(), (n, bits)  # nothing above `bits`
            if name == "uniform" and n >= 2048:
                assert len(np.unique(k)) >= min(int(m) + 1, 1500) * 0.9, (n, bits)
                assert (np.bincount((k & np.uint32(63)).astype(np.int64), minlength=64) > 0).sum() == min(int(m) + 1, 64)  # every digit occurs
            if name == "all_equal":
                assert (k == k[0]).all()
            if name == "two_values":
                assert (k[0::2] == m).all() and (k[1::2] == m >> np.uint32(1)).all() and (n < 2 or k[0] > k[1])
            if name == "sorted":
                assert (np.diff(k.astype(np.int64)) >= 0).all()
            if name == "reversed":
                assert (np.diff(k.astype(np.int64)) <= 0).all() and (n < 64 or bits < 6 or k[0] > k[-1])
            if name == "runs":
                r = _runs(k)
                assert len(np.unique(k)) <= SP.RUN_KEYS and (r[:-1] >= SP.RUN_MIN).all(), (n, bits)  # (the last run is cut off at n)
                if n >= 2048 and bits >= 5:
                    assert len(r) >= 4 and len(np.unique(k)) >= 2, (n, bits)  # several runs, so a wave holds one digit and a tile several
            if name == "high_bits" and n >= 63:
                assert (k & ~m).any() and not np.array_equal(SP.radix_order(k, bits), SP.radix_order(k, 32)), (n, bits)  # masked order != full-key order
            if name == "top_digit":
                assert k[0] >> np.uint32(31) == 1 and (n < 63 or 0.25 < (k >> np.uint32(31)).mean() < 0.75)
                if n >= 63:  # as the first ignored bit it must order nothing: the 31-bit order is not the full-key order
                    assert not np.array_equal(SP.radix_order(k, 31), SP.radix_order(k, 32)), (n, bits)


def _counting_sort(k, bits, count):
    """The radix sort restated: least-significant-digit passes of 6 bits, each a stable counting sort, the last digit cut at `bits`."""
    k = [int(x) for x in k[:count]]
    order = list(range(len(k)))
    for shift in range(0, bits, 6):
        dm = (1 << min(6, bits - shift)) - 1
        bins = [[] for _ in range(64)]
        for i in order:
            bins[(k[i] >> shift) & dm].append(i)
        order = [i for b in bins for i in b]
    return np.array(order, np.int32)


def test_references_agree_with_their_restatements():
    for name in SP.KEY_CLASSES:
        for n in (1, 2, 65, 600):
            for bits in SP.RADIX_BITS:
                if SP.applies(name, bits):
                    k = SP.keys(name, n, bits)
                    for count in {n, n // 2}:
                        assert np.array_equal(SP.radix_order(k, bits, count), _counting_sort(k, bits, count)), (name, n, bits, count)
    rng = np.random.default_rng(5)
    for n in (1, 3, 1025):
        k = SP.with_max(SP.keys("runs", n, 32))
        idx = rng.permutation(n).astype(np.int32)
        o = SP.small_order(k, idx)
        assert o.tolist() == sorted(range(n), key=lambda i: (int(k[i]), int(idx[i])))
        assert k[0] == 0xFFFFFFFF and k[o][-1] == 0xFFFFFFFF
    node = np.array([7, -1, 3, 7, -5, 0, 3], np.int32)
    assert SP.side_keys(node, 7).tolist() == [7, 0xFFFFFFFF, 3, 7, 0xFFFFFFFF, 0, 3]
    ks, o = SP.side_order(node, 7)
    assert o.tolist() == [5, 2, 6, 0, 3, 1, 4] and ks.tolist() == [0, 3, 3, 7, 7, 0xFFFFFFFF, 0xFFFFFFFF]
    ks, o = SP.side_order(None, 4)
    assert o.tolist() == [0, 1, 2, 3] and not ks.any()
    nd = SP.nodes(20000)
    assert 3500 < len(np.unique(nd)) <= 4001 and 0.03 < (nd < 0).mean() < 0.07 and np.bincount(np.unique(nd[nd >= 0], return_inverse=True)[1]).max() < 30


def test_case_lists():
    assert SP.counts(2049) == [0, 1, 2047, 2048, 2049] and SP.counts(50000) == [0, 1, 2047, 2048, 2049, 49999, 50000]
    tile, bins, scan_single = 256 * 8, 64, 16384  # RS_TILE, RS_BINS, SCAN_SINGLE_MAX of csrc/sv_sort.hip
    lo, hi = SP.RADIX_SCAN_SWITCH
    assert bins * -(-lo // tile) == scan_single and bins * -(-hi // tile) > scan_single and hi == lo + 1
    src = (ROOT / "stella_vslam_amd" / "csrc" / "sv_sort.hip").read_text() + (ROOT / "stella_vslam_amd" / "csrc" / "sv_sort.h").read_text()
    for text in ("#define RS_BITS 6", "#define RS_THREADS 256", "#define RS_ITEMS 8", "#define SCAN_SINGLE_MAX 16384", f"#define SV_SORT_SMALL_MAX {SP.SMALL_MAX}"):
        assert text in src, text
    assert SP.SMALL_MAX in SP.SMALL_N and SP.SMALL_MAX in SP.SIDES_N and SP.SMALL_MAX + 1 in SP.SIDES_N and SP.SMALL_MAX + 1 in SP.BUCKET_N
    assert 4096 * 8 <= 48 * 1024 < 8192 * 8 and {4096, 4097} <= set(SP.SMALL_N)  # 4 097 composites pad to 8 192: the first size beyond 48 KB


def test_wrong_variants_are_caught():
    """Every class listed for a wrong sort tells it from the right one, at every size of at least two runs and every `bits` it applies to."""
    for wrong, classes in SP.EXPOSES.items():
        for name in classes:
            for n in [x for x in ALL_N if x >= 2 * SP.RUN_MIN]:
                for bits in SP.RADIX_BITS:
                    if not SP.applies(name, bits) or (wrong == "full_key" and bits == 32) or (n in SP.RADIX_SCAN_SWITCH and bits != 13):
                        continue  # (the two large sizes: at the one `bits` the GPU test runs them with)
                    for count in ([c for c in SP.counts(n) if 2 * SP.RUN_MIN <= c < n] if wrong == "ignore_count" else [n]):
                        k = SP.counted(name, n, count, bits)
                        assert np.array_equal(k[:count], SP.keys(name, n, bits)[:count]) and not k[count:].any()
                        right, bad = SP.radix_order(k, bits, count), SP.WRONG[wrong](k, bits, count)
                        assert len(bad) == len(right) and not np.array_equal(bad, right), (wrong, name, n, bits, count)
    # and the right sort is none of them where they differ at all: a class outside a list need not expose the fault, but must not be "caught"
    k = SP.keys("sorted", 2049, 13)
    assert np.array_equal(SP.WRONG["full_key"](k, 13), SP.radix_order(k, 13))
