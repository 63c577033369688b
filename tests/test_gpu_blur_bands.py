"""GPU parity of the batch blur (k_blur<BLUR_ROWS>: row bands staged in LDS) against the CPU oracle's cv::GaussianBlur 7x7, byte for byte.

A context configured for more than BLUR_SMALL_BATCH frames takes the band kernel whatever the size of the batch it is given, so the
single-frame entry point of an extractor built with max_batch = 5 runs it.  The oracle blurs the pyramid levels the device itself
produced (tests/test_gpu_orb.py compares those with the oracle's pyramid): this file is about the blur alone.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from stella_vslam_amd import synthetic as S

pytestmark = pytest.mark.gpu

# mirrors of stella_vslam_amd/csrc/orb_plan.h (test_constants_mirror_the_header reads the header)
BLUR_ROWS = 48        # output rows of a band
BLUR_SMALL_BATCH = 4  # contexts of at most this many frames keep the streaming kernel
MAX_BATCH = BLUR_SMALL_BATCH + 1

# the sizes of tests/test_gpu_orb.py, then sizes added until test_level_sizes_cover_the_band_geometry holds
SIZES = [(640, 480), (752, 480), (1241, 376), (320, 240), (203, 157), (131, 100), (331, 250), (1920, 1080),
         (60, 168), (128, 176), (256, 194), (512, 236), (515, 130)]


@pytest.fixture(scope="module")
def F():
    from stella_vslam_amd import feature
    return feature


def _extractor(F):
    return F.orb_extractor(F.orb_params(), max_batch=MAX_BATCH)


def _assert_blur_matches(ext, what):
    pyr = ext.image_pyramid_
    for l, a in enumerate(ext.blurred_pyramid()):
        assert np.array_equal(a, O.gaussian_blur7(pyr[l])), f"{what}: blurred level {l} ({a.shape[1]}x{a.shape[0]})"


def test_constants_mirror_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stella_vslam_amd", "csrc", "orb_plan.h")).read()
    assert int(re.search(r"^#define BLUR_ROWS (\d+)", hdr, flags=re.M).group(1)) == BLUR_ROWS
    assert int(re.search(r"^#define BLUR_SMALL_BATCH (\d+)", hdr, flags=re.M).group(1)) == BLUR_SMALL_BATCH


def test_level_sizes_cover_the_band_geometry(F):
    """The level sizes of SIZES, as the library reports them, contain every case the band kernel distinguishes (R = BLUR_ROWS)."""
    R = BLUR_ROWS
    sizes = []
    for w, h in SIZES:
        ext = _extractor(F)
        ext._configure(w, h)
        lv = [ext.level_size(l) for l in range(ext.orb_params_.num_levels_)]
        print((w, h), lv)
        sizes += [s for s in lv if s[0] >= 16]  # narrower levels belong to k_blur_gather
    ws, hs = {w for w, _ in sizes}, {h for _, h in sizes}
    assert {w % 4 for w in ws} == {0, 1, 2, 3}
    assert any(16 <= w <= 20 for w in ws), "a width just above 16"
    for X in (128, 256, 512):  # 32 / 64 / 128 column groups: half a wave, one wave, two waves -- and one group more
        assert any(X - 3 <= w <= X for w in ws) and any(X < w <= X + 4 for w in ws), f"widths around {X}"
    assert 1241 in ws and 1920 in ws
    for h in (R - 1, R, R + 1, R + 6):
        assert h in hs, f"height {h}"
    assert any(R + 1 < h < R + 6 for h in hs), "a second band of 2 .. 5 rows (below R + 7)"
    assert any(h >= 2 * R and 1 <= h % R < 6 for h in hs), "full bands, then a last band shorter than its halo"


@pytest.mark.parametrize("w,h", SIZES)
def test_blurred_levels_bit_exact(F, w, h):
    ext = _extractor(F)
    ext.extract(S.frame(w, h, 100 + w))
    _assert_blur_matches(ext, f"{w}x{h}")


def test_same_frame_after_another_frame(F):
    """What an earlier frame left behind in LDS or in the blurred buffer does not reach the result: a frame, a different frame, the first again."""
    ext = _extractor(F)
    a, b = S.frame(640, 480, 1), 255 - S.frame(640, 480, 2)
    ext.extract(a)
    first = ext.blurred_pyramid()
    ext.extract(b)
    _assert_blur_matches(ext, "second frame")
    ext.extract(a)
    again = ext.blurred_pyramid()
    for l, (x, y) in enumerate(zip(first, again)):
        assert np.array_equal(x, y), f"level {l}"
    _assert_blur_matches(ext, "first frame again")


@pytest.mark.parametrize("w,h", [(640, 480), (331, 250)])
def test_batch_of_three_frames(F, w, h):
    """Three distinct device-resident frames in one call, each compared on its own (frame -> XCD mapping, per-frame offsets)."""
    import torch
    from stella_vslam_amd._lib import lib
    L = lib()
    B = 3
    p = F.orb_params()
    NL = p.num_levels_
    ctx = F.Context(0)
    ctx.check(L.svgpu_orb_configure(ctx.handle, w, h, MAX_BATCH, C.c_float(p.scale_factor_), NL, p.ini_fast_thr_, p.min_fast_thr_, C.c_uint(800)), "cfg")
    cap = max(L.svgpu_orb_max_keypoints(ctx.handle), 1)
    imgs = [S.frame(w, h, 40 + i) for i in range(B)]
    stride = (w + 3) & ~3
    host = np.zeros((B, h, stride), np.uint8)
    for i, im in enumerate(imgs):
        host[i, :, :w] = im
    dev = torch.from_numpy(host).cuda()
    kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(B * (1 + NL), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(L.svgpu_orb_extract_batch_device(ctx.handle, C.c_void_p(dev.data_ptr()), B, C.c_size_t(h * stride), stride, None, C.c_size_t(0), 0,
                                               C.c_void_p(kps.data_ptr()), C.c_void_p(desc.data_ptr()), cap, C.c_void_p(counts.data_ptr()), None), "extract")
    ctx.synchronize()
    for i in range(B):
        for l in range(NL):
            lw, lh = C.c_int(), C.c_int()
            ctx.check(L.svgpu_orb_level_size(ctx.handle, l, C.byref(lw), C.byref(lh)), "level_size")
            src = np.zeros((lh.value, lw.value), np.uint8)
            out = np.zeros_like(src)
            ctx.check(L.svgpu_orb_pyramid_download(ctx.handle, i, l, src.ctypes.data_as(C.c_void_p), lw.value), "pyramid_download")
            ctx.check(L.svgpu_orb_blurred_download(ctx.handle, i, l, out.ctypes.data_as(C.c_void_p), lw.value), "blurred_download")
            if l == 0:
                assert np.array_equal(src, imgs[i])
            assert np.array_equal(out, O.gaussian_blur7(src)), f"frame {i} level {l}"
