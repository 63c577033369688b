"""GPU parity at the edges of ORB extraction: the min_fast_thr retry pass of k_fast, both sides of the strict `A > t` threshold test
and threshold 0, masks on the batch-device path, independence of a frame's results from its neighbours in the batch, and random
extractor geometries -- every case against the CPU oracle (pyramid, blurred levels, level counts, keypoints, descriptors), through
both describe kernels (k_describe_bands and the per-keypoint k_describe).  Images: tests/orb_images.py."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import orb_images as OI

pytestmark = pytest.mark.gpu

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
DESCRIBE = ("bands", "legacy")


@pytest.fixture(scope="module")
def F():
    from stella_vslam_amd import feature
    return feature


@contextlib.contextmanager
def _describe(kind):
    """SVGPU_DESCRIBE_BANDS (read at every launch) forces k_describe_bands; SVGPU_DESCRIBE_LEGACY (read by svgpu_orb_configure) forces
    k_describe.  Both are restored afterwards."""
    saved = {k: os.environ.pop(k, None) for k in ("SVGPU_DESCRIBE_LEGACY", "SVGPU_DESCRIBE_BANDS")}
    os.environ["SVGPU_DESCRIBE_BANDS" if kind == "bands" else "SVGPU_DESCRIBE_LEGACY"] = "1"
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _assert_same(kg, dg, ko, do, what=""):
    assert len(kg) == len(ko), (what, len(kg), len(ko))
    for f in KP_FIELDS:
        assert np.array_equal(kg[f], ko[f]), (what, f)
    assert np.array_equal(dg, do), what


def _oracle(img, mask=None, sf=1.2, nl=8, ini=20, mn=7, area=800):
    return O.orb_extract(img, mask=mask, scale_factor=sf, num_levels=nl, ini_thr=ini, min_thr=mn, min_area=area, cap=60000, want_pyramid=True)


def _check_levels(pyr_dl, blur_dl, pyr, what=""):
    for l, (a, b) in enumerate(zip(pyr_dl, pyr)):
        assert np.array_equal(a, b), (what, "pyramid level", l)
    for l, a in enumerate(blur_dl):
        assert np.array_equal(a, O.gaussian_blur7(pyr[l])), (what, "blurred level", l)


def _single(F, img, kind, mask=None, sf=1.2, nl=8, ini=20, mn=7, area=800):
    """svgpu_orb_extract (one frame, host in / host out) against the oracle; returns the oracle's keypoints."""
    with _describe(kind):
        ext = F.orb_extractor(F.orb_params("edges", sf, nl, ini, mn), min_area=area)
        kg, dg = ext.extract(img, mask)
    ko, do, counts, pyr = _oracle(img, mask, sf, nl, ini, mn, area)
    what = (kind, img.shape, sf, nl, ini, mn)
    _check_levels(ext.image_pyramid_, ext.blurred_pyramid(), pyr, what)
    assert np.array_equal(ext.level_counts_, counts), what
    _assert_same(kg, dg, ko, do, what)
    return ko


def _batch(F, frames, kind, masks=None, sf=1.2, nl=8, ini=20, mn=7, area=800, pad=0, off=0, mpad=0, moff=0, ctx=None, download=True):
    """svgpu_orb_extract_batch_device on device-resident frames: rows `w + pad` bytes apart, base `off` bytes past an aligned address,
    frame stride off a multiple of 4 when pad is.  `masks`: None, one (h, w) array shared by every frame (mask_frame_stride 0) or
    (B, h, w) per frame, rows `w + mpad` apart at `moff` bytes past an aligned base.  Returns per frame (keypoints, descriptors,
    counts [total, per level], pyramid, blurred) -- pyramid / blurred only with `download`."""
    import torch
    from stella_vslam_amd._lib import lib
    L = lib()
    B, h, w = frames.shape
    with _describe(kind):
        if ctx is None:
            ctx = F.Context(0)
            ctx.check(L.svgpu_orb_configure(ctx.handle, w, h, B, C.c_float(sf), nl, ini, mn, C.c_uint(area)), "cfg")
        cap = max(L.svgpu_orb_max_keypoints(ctx.handle), 1)
        stride = w + pad
        fstride = h * stride + (pad & 1)
        host = np.zeros(off + B * fstride + 64, np.uint8)
        for b in range(B):
            host[off + b * fstride: off + b * fstride + h * stride].reshape(h, stride)[:, :w] = frames[b]
        img = torch.from_numpy(host).cuda()
        mdev, mfs, mpitch = None, 0, 0
        if masks is not None:
            mk = masks[None] if masks.ndim == 2 else masks
            mpitch = w + mpad
            mfs = 0 if masks.ndim == 2 else h * mpitch + 1
            mh = np.full(moff + len(mk) * max(mfs, h * mpitch) + 64, 0xEE, np.uint8)
            for b in range(len(mk)):
                mh[moff + b * mfs: moff + b * mfs + h * mpitch].reshape(h, mpitch)[:, :w] = mk[b]
            mdev = torch.from_numpy(mh).cuda()
        kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
        desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(B * (1 + nl), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.check(L.svgpu_orb_extract_batch_device(ctx.handle, C.c_void_p(img.data_ptr() + off), B, C.c_size_t(fstride), stride,
                                                   None if mdev is None else C.c_void_p(mdev.data_ptr() + moff), C.c_size_t(mfs), mpitch,
                                                   C.c_void_p(kps.data_ptr()), C.c_void_p(desc.data_ptr()), cap,
                                                   C.c_void_p(counts.data_ptr()), None), "extract")
        ctx.synchronize()
    kk = kps.cpu().numpy().view(O.KEYPOINT_DTYPE).reshape(B, cap)
    dd = desc.cpu().numpy().reshape(B, cap, 32)
    cc = counts.cpu().numpy().reshape(B, 1 + nl)
    out = []
    for b in range(B):
        n = int(cc[b, 0])
        assert n <= cap
        pyr = blur = None
        if download:
            pyr, blur = [], []
            for l in range(nl):
                lw, lh = C.c_int(), C.c_int()
                ctx.check(L.svgpu_orb_level_size(ctx.handle, l, C.byref(lw), C.byref(lh)), "level_size")
                a, z = np.zeros((lh.value, lw.value), np.uint8), np.zeros((lh.value, lw.value), np.uint8)
                ctx.check(L.svgpu_orb_pyramid_download(ctx.handle, b, l, a.ctypes.data_as(C.c_void_p), lw.value), "pyr")
                ctx.check(L.svgpu_orb_blurred_download(ctx.handle, b, l, z.ctypes.data_as(C.c_void_p), lw.value), "blur")
                pyr.append(a)
                blur.append(z)
        out.append((kk[b, :n].copy(), dd[b, :n].copy(), cc[b].copy(), pyr, blur))
    return out


def _check_batch(res, frames, masks=None, sf=1.2, nl=8, ini=20, mn=7, area=800, what=""):
    for b, (k, d, c, pyr, blur) in enumerate(res):
        m = None if masks is None else (masks if masks.ndim == 2 else masks[b])
        ko, do, counts, opyr = _oracle(frames[b], m, sf, nl, ini, mn, area)
        if pyr is not None:
            _check_levels(pyr, blur, opyr, (what, b))
        assert np.array_equal(c[1:], counts), (what, b, c, counts)
        _assert_same(k, d, ko, do, (what, b))


# ----------------------------------------------------------------------------------------------------------- 1. image classes
@pytest.mark.parametrize("kind", DESCRIBE)
@pytest.mark.parametrize("name", list(OI.CLASSES))
def test_image_classes_single_frame(F, name, kind):
    """k_pyramid_lds, k_blur, k_fast (both passes: the checkerboards at d = 8 and 20 and the low-contrast classes take the
    min_thr retry), k_select and the describe kernel on every image class of tests/orb_images.py."""
    _single(F, OI.CLASSES[name](), kind)


# ----------------------------------------------------------------------------------------------------------- 2. thresholds
@pytest.mark.parametrize("kind", DESCRIBE)
@pytest.mark.parametrize("ini,mn", [(20, 7), (20, 1), (20, 0), (1, 1), (0, 0), (12, 12), (60, 20)])
@pytest.mark.parametrize("name", ["low_contrast", "spots"])
def test_fast_thresholds(F, name, ini, mn, kind):
    """k_fast's quick test, arc score and NMS at thresholds 0 and 1 (cv::FAST gives a corner of arc score 1 the NMS score 0 at
    threshold 0: it never beats a neighbour), a retry at the same threshold (12 / 12) and a high first pass (60 / 20)."""
    ko = _single(F, OI.CLASSES[name](), kind, ini=ini, mn=mn)
    if name == "spots" and min(ini, mn) <= 1:
        assert len(ko) > 0


# ----------------------------------------------------------------------------------------------------------- 3. masks, batch path
def _masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.ones((4, h, w), np.uint8)
    m[0][(xx - w // 2) ** 2 + (yy - h // 3) ** 2 <= (h // 4) ** 2] = 0
    m[1][3 * h // 4:] = 0
    m[1][:, :w // 5] = 0
    m[2][h // 5:h // 2, w // 3:2 * w // 3] = 0
    rng = np.random.default_rng(17)
    for _ in range(12):
        y, x = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
        m[3][y:y + 40, x:x + 40] = 0
    m[2] *= 255  # any non-zero value is "keep"
    return m


def _mixed_frames(w=640, h=480):
    return np.stack([OI.low_contrast(w, h, 1), OI.checkerboard(w, h, 20), OI.half_low_contrast(w, h, 2), OI.symmetric_motifs(w, h, 3)])


@pytest.mark.parametrize("kind", DESCRIBE)
@pytest.mark.parametrize("mpad,moff", [(0, 0), (3, 1), (5, 2)])
def test_batch_masks_per_frame(F, kind, mpad, moff):
    """k_fast's mask tests (cell corners, then each keypoint) with one mask per frame of a batch of four mixed classes, at mask
    row pitches that are not a multiple of 4 (643, 645) and mask base addresses off alignment."""
    frames, masks = _mixed_frames(), _masks(480, 640)
    res = _batch(F, frames, kind, masks=masks, mpad=mpad, moff=moff, pad=mpad, off=moff)
    _check_batch(res, frames, masks, what=(kind, mpad, moff))
    assert all(len(r[0]) > 0 for r in res)


@pytest.mark.parametrize("kind", DESCRIBE)
def test_batch_mask_shared(F, kind):
    """mask_frame_stride = 0: one mask serves every frame of the batch (k_fast reads it at the same address for each frame)."""
    frames, masks = _mixed_frames(), _masks(480, 640)
    res = _batch(F, frames, kind, masks=masks[0], mpad=1, moff=3)
    _check_batch(res, frames, masks[0], what=kind)


@pytest.mark.parametrize("kind", DESCRIBE)
def test_mask_applied_after_the_retry_decision(F, kind):
    """orb_extractor.cc:228-256 decides on the min_thr retry BEFORE the keypoint mask: a cell whose every ini_thr corner lies in a
    masked hole (its four corners left unmasked) yields nothing.  A k_fast that masked first would retry and emit min_thr corners."""
    img = OI.low_contrast(640, 480, 1)
    mask, cells = OI.mask_retry_holes(img, O.fast9_16)
    assert len(cells) >= 3
    ko = _single(F, img, kind, mask=mask)
    for (x0, y0, x1, y1) in cells:  # nothing of level 0 comes from those cells' scored area but the neighbours' overlap
        inside = (ko["octave"] == 0) & (ko["x"] >= x0 + 9) & (ko["x"] < x1 - 9) & (ko["y"] >= y0 + 9) & (ko["y"] < y1 - 9)
        assert not inside.any()
    frames = np.stack([img, OI.low_contrast(640, 480, 4), img])
    masks = np.stack([mask, np.ones_like(mask), mask])
    _check_batch(_batch(F, frames, kind, masks=masks, mpad=3, moff=1, download=False), frames, masks, what=kind)


# ----------------------------------------------------------------------------------------------------------- 4. neighbours and position
@pytest.mark.parametrize("kind", DESCRIBE)
@pytest.mark.parametrize("w,h", [(621, 429), (622, 430), (677, 485)])  # (w - 38) % 64, (h - 38) % 64 = 7, 8, 63: partial edge cells
def test_probe_independent_of_batch_neighbours_and_position(F, kind, w, h):
    """k_fast stages only the cell's own rows and pieces into LDS (what a previous cell or workgroup left there stays): a probe frame
    with retried and plain cells and partial edge cells gives the same bytes in batches of 1, 4 and 8 among all-255, all-0 and noise
    frames, at every position of the batch, and equals the oracle."""
    from stella_vslam_amd._lib import lib
    L = lib()
    probe = OI.probe(w, h)
    fill = [np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8), OI.noise(w, h, 9)]
    with _describe(kind):
        ctx = F.Context(0)
        ctx.check(L.svgpu_orb_configure(ctx.handle, w, h, 8, C.c_float(1.2), 8, 20, 7, C.c_uint(800)), "cfg")
    ref = _batch(F, probe[None], kind, ctx=ctx)[0]
    _check_batch([ref], probe[None], what=(kind, w, h))
    assert (ref[0]["response"] < 20).sum() > 20  # the retry pass contributes
    for B in (4, 8):
        for pos in range(B):
            frames = np.stack([fill[(pos + i) % 3] for i in range(B)])
            frames[pos] = probe
            k, d, c, _, _ = _batch(F, frames, kind, ctx=ctx, pad=B - 3, off=pos % 4, download=False)[pos]
            assert np.array_equal(c, ref[2]), (B, pos)
            assert np.array_equal(k.view(np.uint8), ref[0].view(np.uint8)) and np.array_equal(d, ref[1]), (B, pos)


# ----------------------------------------------------------------------------------------------------------- 5. random geometries
def test_random_geometries_against_the_oracle(F):
    """Every stage against the oracle (not only one describe kernel against the other) on twelve seeded draws: scale factor
    1.1..2.0, 1..12 levels (each at least 45 px wide and high), FAST thresholds 0..60 with min <= ini, an image class per frame,
    batch 1..3, row stride and base address off alignment."""
    rng = np.random.default_rng(20261016)
    names = list(OI.CLASSES)
    total = 0
    for draw in range(12):
        w, h = int(rng.integers(120, 1000)), int(rng.integers(100, 600))
        sf = float(rng.choice([1.1, 1.2, 1.3, 1.5, 2.0]))
        nl = int(rng.integers(1, 13))
        while nl > 1 and min(O.level_sizes(w, h, sf, nl)[-1]) < 45:
            nl -= 1
        ini = int(rng.integers(0, 61))
        mn = int(rng.integers(0, ini + 1))
        area = int(rng.choice([200, 800, 2000]))
        B, pad, off = int(rng.integers(1, 4)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        frames = np.stack([OI.make(names[int(rng.integers(len(names)))], w, h, int(rng.integers(1 << 12))) for _ in range(B)])
        for kind in DESCRIBE:
            res = _batch(F, frames, kind, sf=sf, nl=nl, ini=ini, mn=mn, area=area, pad=pad, off=off, download=kind == "bands")
            _check_batch(res, frames, sf=sf, nl=nl, ini=ini, mn=mn, area=area, what=(draw, kind, w, h, sf, nl, ini, mn, area, B, pad, off))
        total += sum(len(r[0]) for r in res)
    assert total > 3000
