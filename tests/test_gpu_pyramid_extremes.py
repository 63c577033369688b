"""k_pyramid_lds against the oracle's cv::resize chain, byte for byte, on images that drive the horizontal sums H and the blended
results v to their bounds (the kernel packs four results into a dword without masking them to a byte: a0 + a1 <= 2049 and
b0 + b1 <= 2049 keep every v <= 255, tests/orb_coef_sum_check.cpp), at sizes whose level 1 has 63, 64 and 65 column groups (a chunk of
rows ends exactly on, just before and just behind a wave boundary), at 640 x 480, and through every level-0 staging path: LDS-DMA
(16-byte aligned rows, pitch equal to and larger than the width), the dword path and the byte path (odd row stride, base address off
4-byte alignment).  One frame through the host entry point and batches of five through the device entry point."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_orb_edges import _batch

pytestmark = pytest.mark.gpu

NL = 8


def _all255(w, h):
    return np.full((h, w), 255, np.uint8)


def _all0(w, h):
    return np.zeros((h, w), np.uint8)


def _checker1(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def _vstripes(w, h):
    return np.ascontiguousarray(np.broadcast_to(((np.arange(w) & 1) * 255).astype(np.uint8), (h, w)))


def _hstripes(w, h):
    return np.ascontiguousarray(np.broadcast_to(((np.arange(h) & 1) * 255).astype(np.uint8)[:, None], (h, w)))


def _edge_rows(w, h):
    img = np.zeros((h, w), np.uint8)
    img[0] = 255
    img[-1] = 255
    return img


CONTENTS = {"all255": _all255, "all0": _all0, "checker1": _checker1, "vstripes": _vstripes, "hstripes": _hstripes, "edge_rows": _edge_rows}

# (w, h, pad, off) of the batch layout: rows w + pad bytes apart, base `off` bytes past an aligned address
SIZES = {
    "groups63": (302, 229, 0, 0),       # level 1: 252 px = 63 column groups; 302-byte rows: the byte path
    "groups64a": (305, 229, 3, 0),      # level 1: 254 px = 64 groups (two pixels of the last one repeat the last column); 308-byte rows: dwords
    "groups64b": (307, 229, 0, 0),      # level 1: 256 px = 64 groups exactly
    "groups65": (312, 229, 0, 0),       # level 1: 260 px = 65 groups; 312-byte rows: the dword path
    "vga": (640, 480, 0, 0),            # LDS-DMA staging, pitch = width
    "vga_strided": (640, 480, 64, 0),   # LDS-DMA staging, 704-byte rows
    "odd_unaligned": (131, 100, 2, 1),  # 133-byte rows, base off 4-byte alignment: the byte path
}


def test_level1_group_counts_are_what_the_names_say():
    for name, groups in (("groups63", 63), ("groups64a", 64), ("groups64b", 64), ("groups65", 65)):
        w, h = SIZES[name][:2]
        assert (O.level_sizes(w, h, 1.2, NL)[1][0] + 3) // 4 == groups, name


@functools.lru_cache(maxsize=None)
def _oracle_pyramid(content, w, h):
    img = CONTENTS[content](w, h)
    levels = [img]
    for (lw, lh) in O.level_sizes(w, h, 1.2, NL)[1:]:
        levels.append(O.resize_linear(levels[-1], lw, lh))
    for a in levels:
        a.setflags(write=False)
    return levels


def _same(got, content, w, h, what):
    ref = _oracle_pyramid(content, w, h)
    assert len(got) == len(ref) == NL
    for l, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and np.array_equal(a, b), (what, content, "level", l, int((a != b).sum()))


def test_extreme_contents_reach_the_bounds():
    """all 255 stays 255 on every level (H and v at their largest), the stripes and the checkerboard blend to values strictly
    between the extremes on level 1."""
    w, h = SIZES["groups64b"][:2]
    assert all((lv == 255).all() for lv in _oracle_pyramid("all255", w, h))
    assert all((lv == 0).all() for lv in _oracle_pyramid("all0", w, h))
    for content in ("checker1", "vstripes", "hstripes"):
        l1 = _oracle_pyramid(content, w, h)[1]
        assert l1.min() < 64 and l1.max() > 191 and ((l1 > 0) & (l1 < 255)).any(), content


@pytest.mark.parametrize("size", list(SIZES))
def test_single_frame(size):
    from stella_vslam_amd import feature as F
    w, h = SIZES[size][:2]
    ext = F.orb_extractor(F.orb_params("pyramid", 1.2, NL, 20, 7))
    for content in CONTENTS:
        ext.extract(CONTENTS[content](w, h))
        _same(ext.image_pyramid_, content, w, h, (size, "single"))


@pytest.mark.parametrize("size", list(SIZES))
def test_batch_of_five(size):
    from stella_vslam_amd import feature as F
    w, h, pad, off = SIZES[size]
    names = list(CONTENTS)
    for first in (0, 1):  # six contents, five frames: two batches cover them at different positions
        batch = [names[(first + i) % len(names)] for i in range(5)]
        frames = np.stack([CONTENTS[c](w, h) for c in batch])
        res = _batch(F, frames, "bands", pad=pad, off=off)
        for b, c in enumerate(batch):
            _same(res[b][3], c, w, h, (size, "batch", first, b))
