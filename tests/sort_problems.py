"""Inputs and numpy references for the device sorts of csrc/sv_sort.hip and the bucket order of csrc/bucket_kernels.hip: numpy only.

Three operations, each with the reference the GPU tests compare against, element for element:
  radix       sv_sort_pairs: STABLE order of the first `count` (key, value) pairs by the low `bits` key bits; whole keys travel with their values
  small       sv_sort_small / sv_sort_small_sides: order by (key, index), the index compared as an unsigned number
  side        the keys a side's node ids become: node < 0 -> 0xFFFFFFFF (behind every bucket), no node ids -> one bucket, identity order

`keys(name, n, bits, seed)` builds the named key class; tests/test_sort_problem_classes.py shows that every class is what it claims and
that three planted wrong sorts (`WRONG`) are told from the right one by the classes listed in `EXPOSES`."""
import numpy as np

KEY_CLASSES = ["uniform", "all_equal", "two_values", "sorted", "reversed", "runs", "high_bits", "top_digit"]
RUN_MIN, RUN_KEYS = 64, 5      # `runs`: at most RUN_KEYS distinct keys, every run but the cut-off last one at least one wave long

# sizes either side of one wave (64), of one radix tile (2 048 = 256 threads x 8) and two tiles; the digit is 6 bits wide: `bits` that end
# inside the first digit, on its edge, one past it, on and past the second edge, and in the last, 2-bit digit of a 32-bit key
RADIX_N = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4096]
RADIX_BITS = [1, 5, 6, 7, 12, 13, 31, 32]
RADIX_SCAN_SWITCH = [524288, 524289]   # 64 bins x 256 / 257 tiles = 16 384 / 16 448 histogram entries: the one-workgroup scan / the tiled one
COUNT_N = [2049, 50000]
COUNT_BITS = [6, 7, 18]
SMALL_MAX = 16384                      # SV_SORT_SMALL_MAX
SMALL_N = [1, 2, 3, 1023, 1024, 1025, 4096, 4097, 8192, 16383, 16384]   # 4 097: the first size whose 8-byte composites pass 48 KB of LDS
SMALL_CLASSES = ["all_equal", "two_values", "runs"]
SIDES_N = [0, 1, 64, 65, 1025, 4097, 16384, 16385]
BUCKET_N = [16384, 16385, 20000]
SENTINEL = 0xA5A5A5A5                  # what svgpu_selftest_sort_paths fills the outputs of the several-sides launch with


def mask(bits):
    return np.uint32(0xFFFFFFFF if bits >= 32 else (1 << bits) - 1)


def applies(name, bits):
    """high_bits needs key bits above `bits`; top_digit is about bit 31 as the first ignored bit (31) and as the top of the last digit (32)"""
    return bits < 32 if name == "high_bits" else bits in (31, 32) if name == "top_digit" else True


def counts(n):
    """element counts of a launch sized for n: none, one, either side of a radix tile, one short of the launch, all of it"""
    return sorted({min(c, n) for c in (0, 1, 2047, 2048, 2049, n - 1, n)})


def keys(name, n, bits, seed=0):
    assert applies(name, bits)
    rng = np.random.default_rng([seed, n, bits, KEY_CLASSES.index(name)])
    m = int(mask(bits))
    low = rng.integers(0, m + 1, n, dtype=np.uint64).astype(np.uint32)
    if name == "uniform":
        return low
    if name == "all_equal":
        return np.full(n, low[0] if n else 0, np.uint32)
    if name == "two_values":  # the larger one first, so that the sorted order is not the input order
        return np.where(np.arange(n) % 2 == 0, np.uint32(m), np.uint32(m >> 1)).astype(np.uint32)
    if name == "sorted":
        return np.sort(low)
    if name == "reversed":
        return np.ascontiguousarray(np.sort(low)[::-1])
    if name == "runs":
        vals = rng.choice(m + 1, min(RUN_KEYS, m + 1), replace=False).astype(np.uint32)  # distinct (all there are where `bits` is small)
        out, have = [], 0
        while have < n:  # (two neighbours with the same key are one longer run)
            out.append(np.full(int(rng.integers(RUN_MIN, 4 * RUN_MIN)), vals[rng.integers(0, len(vals))], np.uint32))
            have += len(out[-1])
        return np.concatenate(out)[:n] if out else np.zeros(0, np.uint32)
    if name == "high_bits":  # garbage above `bits`: it must travel with the key and order nothing
        junk = rng.integers(0, 1 << (32 - bits), n, dtype=np.uint64).astype(np.uint32)
        return (low | (junk << np.uint32(bits))).astype(np.uint32)
    if name == "top_digit":  # bit 31 on about half of the keys (and on the first one)
        top = rng.integers(0, 2, n, dtype=np.uint64).astype(np.uint32)
        top[:1] = 1
        return ((low & np.uint32(0x7FFFFFFF)) | (top << np.uint32(31))).astype(np.uint32)
    raise KeyError(name)


def counted(name, n, count, bits, seed=0):
    """keys of a launch sized for n of which only the first `count` are live: behind them lies the smallest key there is, so that a sort
    which reads beyond the count pulls stale entries to the front of its result"""
    k = keys(name, n, bits, seed)
    k[count:] = 0
    return k


def with_max(k, seed=0):
    """the same keys with about a tenth of them (and the first) replaced by 0xFFFFFFFF, the key of a keypoint without a node"""
    rng = np.random.default_rng([seed, len(k)])
    out = k.copy()
    out[rng.uniform(0, 1, len(k)) < 0.1] = 0xFFFFFFFF
    out[:1] = 0xFFFFFFFF
    return out


# ------------------------------------------------------------------------------------------------ references
def radix_order(k, bits, count=None):
    """positions of the first `count` pairs in sorted order: stable, by the low `bits` key bits"""
    k = np.asarray(k, np.uint32)[:len(k) if count is None else count]
    return np.argsort(k & mask(bits), kind="stable").astype(np.int32)


def small_order(k, idx):
    """positions in (key, index) order"""
    return np.lexsort((np.asarray(idx).astype(np.uint32), np.asarray(k, np.uint32))).astype(np.int32)


def side_keys(node, n):
    if node is None:
        return np.zeros(n, np.uint32)
    node = np.asarray(node, np.int32)
    return np.where(node < 0, np.uint32(0xFFFFFFFF), node.astype(np.uint32)).astype(np.uint32)


def side_order(node, n):
    """(sorted keys, keypoint indices) of one side: by (node id, index), keypoints without a node last, no node ids = identity"""
    k = side_keys(node, n)
    o = small_order(k, np.arange(n))
    return k[o], o


def nodes(n, distinct=4000, negative=0.05, seed=0):
    """node ids of n keypoints: about `distinct` different ids spread over the 32-bit positive range, about `negative` of them -1"""
    rng = np.random.default_rng([seed, n, distinct])
    ids = rng.integers(0, 1 << 31, distinct, dtype=np.int64).astype(np.int32)
    node = ids[rng.integers(0, distinct, n)]
    node[rng.uniform(0, 1, n) < negative] = -1
    return node.astype(np.int32)


# ------------------------------------------------------------------------------------------------ planted wrong sorts
def _unstable(k, bits, count=None):  # right keys, equal keys in falling index order
    k = np.asarray(k, np.uint32)[:len(k) if count is None else count]
    return np.lexsort((-np.arange(len(k)), k & mask(bits))).astype(np.int32)


def _full_key(k, bits, count=None):  # orders by the bits above `bits` too
    return radix_order(k, 32, count)


def _ignore_count(k, bits, count=None):  # sorts everything the launch was sized for and hands back the first `count`
    return radix_order(k, bits)[:len(k) if count is None else count]


WRONG = {"unstable": _unstable, "full_key": _full_key, "ignore_count": _ignore_count}
# the classes that must tell each wrong sort from the right one (at n >= 2 x RUN_MIN; ignore_count: on `counted` keys with 2 x RUN_MIN <= count < n)
EXPOSES = {"unstable": ["all_equal", "two_values", "runs"], "full_key": ["high_bits", "top_digit"],
           "ignore_count": ["uniform", "two_values", "reversed", "runs", "high_bits"]}
