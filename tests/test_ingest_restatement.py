"""Image ingest without a device: the ABI is exported and refuses instead of crashing, and the numpy restatement (tests/ingest_problems.py)
gives the hand-derived values of OpenCV's 8-bit cvtColor / remap / convertTo arithmetic."""
import ctypes as C
import pathlib
import re

import numpy as np

from tests import ingest_problems as IP

ROOT = pathlib.Path(__file__).resolve().parent.parent
F32 = np.float32


def _ingest_names():
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    names = sorted(set(re.findall(r"^(?:int|void)\s+(svgpu_ingest_[a-z0-9_]+|svgpu_tracker_set_ingest)\s*\(", hdr, flags=re.M)))
    return names


def test_header_names_are_exported_and_refuse_without_a_device():
    from stella_vslam_amd._lib import lib
    L = lib()
    names = _ingest_names()
    assert {"svgpu_ingest_create", "svgpu_ingest_destroy", "svgpu_ingest_gray", "svgpu_ingest_gray_batch_device", "svgpu_ingest_depth",
            "svgpu_ingest_depth_device", "svgpu_tracker_set_ingest"} <= set(names)
    for n in names:
        getattr(L, n)
    # no context (what a machine without a device leaves a caller with): every entry point returns an error, none touches its arguments
    h = C.c_void_p()
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    assert L.svgpu_ingest_create(None, 4, 4, 3, IP.RGB, None, None, 0, C.byref(h)) != 0 and not h.value
    assert L.svgpu_ingest_gray(None, None, p, 12, p, 4) != 0
    assert L.svgpu_ingest_gray_batch_device(None, None, p, 1, 48, 12, p, 16, 4, None) != 0
    assert L.svgpu_ingest_depth(None, p, IP.DEPTH_U16, 8, 4, 4, 5000.0, p, 16) != 0
    assert L.svgpu_ingest_depth_device(None, p, IP.DEPTH_U16, 8, 4, 4, 5000.0, p, 16, None) != 0
    assert L.svgpu_tracker_set_ingest(None, None, None, 0, 1.0) != 0
    L.svgpu_ingest_destroy(None)
    assert not buf.any()


def test_grey_hand_values():
    white = np.full((2, 3, 3), 255, np.uint8)
    assert (IP.to_gray(white, IP.RGB) == 255).all() and (IP.to_gray(white, IP.BGR) == 255).all()
    red = np.zeros((1, 1, 3), np.uint8)
    red[..., 0] = 255
    assert IP.to_gray(red, IP.RGB)[0, 0] == 76      # (255 * 9798 + 16384) >> 15
    assert IP.to_gray(red, IP.BGR)[0, 0] == 29      # (255 * 3735 + 16384) >> 15
    green = np.zeros((1, 1, 4), np.uint8)
    green[..., 1], green[..., 3] = 255, 200
    assert IP.to_gray(green, IP.RGB)[0, 0] == IP.to_gray(green, IP.BGR)[0, 0] == 150   # (255 * 19235 + 16384) >> 15; alpha ignored
    g = IP.noise_image(7, 5, 1, 1)
    assert np.array_equal(IP.to_gray(g, IP.GRAY), g) and np.array_equal(IP.to_gray(g[..., None], IP.RGB), g)
    assert IP.CR + IP.CG + IP.CB == 1 << 15
    for bad in (np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 4), np.uint8)):
        try:
            IP.to_gray(bad, IP.GRAY)
        except ValueError:
            continue
        raise AssertionError("Gray with colour channels must be refused")


def test_remap_hand_values():
    img = IP.noise_image(19, 11, 3, 2)
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(F32)
    assert np.array_equal(IP.remap(img, xx, yy), img)                      # identity
    sh = IP.remap(img, xx + F32(3), yy - F32(2))                          # integer shift, zero border
    exp = np.zeros_like(img)
    exp[2:, :w - 3] = img[:h - 2, 3:]
    assert np.array_equal(sh, exp)
    half = IP.remap(img[..., 0], xx + F32(0.5), yy)                       # x + 0.5: (a + b + 1) >> 1, the last column has b outside = 0
    a = img[..., 0].astype(np.int32)
    b = np.concatenate([a[:, 1:], np.zeros((h, 1), np.int32)], 1)
    assert np.array_equal(half, ((a + b + 1) >> 1).astype(np.uint8))
    # 2.515625 = 80.5 / 32: half to even, sx = 80 -> ix = 2, fx = 16 ; 2.546875 = 81.5 / 32 -> 82
    ix, fx, ok = IP.fixed_point(np.array([2.515625, 2.546875, -0.515625], F32))
    assert ok.all() and (ix * 32 + fx).tolist() == [80, 82, -16]
    # entirely outside, non-finite and huge entries give 0 in every channel
    for v in (-5.0, float(w + 3), np.nan, np.inf, -np.inf, 1e9, -1e9):
        assert not IP.remap(img, np.full((h, w), v, F32), yy).any(), v
        assert not IP.remap(img, xx, np.full((h, w), v, F32)).any(), v
    # ... while an entry just across the border still sees the border pixel with its weight
    edge = IP.remap(img[..., 1], np.full((1, 1), -0.25, F32), np.zeros((1, 1), F32))
    assert edge[0, 0] == (int(img[0, 0, 1]) * 24 * 32 * 32 + (1 << 14)) >> 15
    f = np.arange(32)
    tot = sum(IP.weights(f[:, None], f[None, :]))
    assert tot.shape == (32, 32) and (tot == 32768).all()                  # all 1024 fraction pairs


def test_depth_hand_values():
    assert IP.true_depth(np.array([[5000]], np.uint16), 5000.0).view(np.uint32)[0, 0] == np.float32(1.0).view(np.uint32)
    d = IP.true_depth(np.array([[0, 65535, 1]], np.uint16), 5000.0)
    s = F32(1.0 / 5000.0)
    assert d.dtype == np.float32 and d[0, 0] == 0 and d[0, 1] == F32(65535) * s and d[0, 2] == s
    assert np.array_equal(IP.true_depth(np.array([[2.5, -1.0]], F32), 1.0), np.array([[2.5, -1.0]], F32))


def test_remap_then_grey_is_not_grey_then_remap():
    """The reference rectifies the image as read and converts afterwards; the two orders differ in the last bit on noise."""
    img = IP.noise_image(64, 48, 3, 3)
    mx, my = IP.make_maps("fractional_shift", 64, 48)
    a = IP.ingest(img, IP.RGB, mx, my)
    b = IP.remap(IP.to_gray(img, IP.RGB), mx, my)
    assert a.shape == b.shape and not np.array_equal(a, b)
    assert np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 2


def test_generators_cover_their_classes():
    w, h = 203, 157
    for kind in IP.MAP_CLASSES:
        mx, my = IP.make_maps(kind, w, h, seed=4)
        assert mx.dtype == my.dtype == np.float32 and mx.shape == my.shape == (h, w)
    mx, my = IP.make_maps("quarter_outside", w, h, seed=4)
    out = (mx < -1) | (mx >= w) | (my < -1) | (my >= h)
    assert 0.15 < out.mean() < 0.35
    mx, my = IP.make_maps("non_finite", w, h, seed=4)
    assert (~np.isfinite(mx)).any() and (~np.isfinite(my)).any()
    mx, my = IP.make_maps("plumb_bob", w, h, seed=4)
    inside = (mx >= 0) & (mx < w - 1) & (my >= 0) & (my < h - 1)
    assert inside.mean() > 0.9 and (np.modf(mx)[0] != 0).mean() > 0.9
    v = IP.strided(IP.noise_image(10, 4, 3, 1), 37)
    assert v.strides == (37, 3, 1)
