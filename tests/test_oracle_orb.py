"""Pins the CPU oracle's ORB front end against everything the reference's own tests hold for it
 plus independent restatements of the OpenCV primitives' published definitions."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from stella_vslam_amd import synthetic as S
from tests import orb_images as OI


# ---- reference test/stella_vslam/feature/orb_params.cc:27-70 (EXPECT_FLOAT_EQ = 4 ulp)
def _float_eq(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32))) <= 4


def test_scale_tables_match_reference_tests():
    n, sf = 10, np.float32(1.26)
    s, inv, sig, isig = O.scale_tables(float(sf), n)
    at = np.float32(1.0)
    for l in range(n):
        assert _float_eq(s[l], np.float32(math.pow(float(sf), l)))
        assert _float_eq(inv[l], np.float32(math.pow(float(np.float32(1.0) / sf), l)))
        assert _float_eq(sig[l], at * at)
        assert _float_eq(isig[l], np.float32(1.0) / (at * at))
        at = sf * at


# ---- reference test/stella_vslam/util/trigonometric.cc:8-20
def test_trig_within_1e3_of_libm():
    for i in range(3600):
        a = i * 0.1 * math.pi / 180.0
        assert abs(O.lib().orc_util_cos(a) - math.cos(a)) < 1e-3
        assert abs(O.lib().orc_util_sin(a) - math.sin(a)) < 1e-3


def test_level_sizes_640x480():
    assert O.level_sizes(640, 480) == [(640, 480), (533, 400), (444, 333), (370, 278), (309, 231), (257, 193), (214, 161),
                                       (179, 134)]


def test_gauss_taps_and_umax():
    assert list(O.gauss_taps(7, 2.0)) == [18, 34, 48, 56, 48, 34, 18]
    assert list(O.umax()) == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_fast_atan2_close_to_atan2():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        y, x = rng.integers(-50000, 50000, 2)
        a = O.lib().orc_fast_atan2(float(y), float(x))
        ref = math.degrees(math.atan2(y, x)) % 360.0
        d = abs(a - ref)
        assert min(d, 360 - d) < 0.3  # OpenCV documents ~0.3 deg accuracy
    assert O.lib().orc_fast_atan2(0.0, 0.0) == 0.0


# ---- independent definition of FAST-9/16 + score + 3x3 strict NMS (numpy, closed form)
_CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
           (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def _arc_scores(img):
    h, w = img.shape
    I = img.astype(np.int32)
    A = np.zeros((h, w), np.int32)  # max over 9-arcs of min signed difference, both signs
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([c - I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in _CIRCLE])  # v - p_k
    best = np.zeros_like(c)
    for k in range(16):
        idx = [(k + m) % 16 for m in range(9)]
        best = np.maximum(best, d[idx].min(0))
        best = np.maximum(best, (-d[idx]).min(0))
    A[3:h - 3, 3:w - 3] = best
    return A


def fast_definition(img, thr):
    h, w = img.shape
    A = _arc_scores(img)
    score = np.where(A > thr, A - 1, 0)
    out = []
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            s = score[y, x]
            if s == 0 and A[y, x] <= thr:
                continue
            nb = score[y - 1:y + 2, x - 1:x + 2].copy()
            nb[1, 1] = -1
            if (s > nb).all():
                out.append((x, y, s))
    return np.array(out, np.int32).reshape(-1, 3)


# threshold 0 (tests/orb_images.py): a corner of arc score 1 gets the NMS score 0, a non-corner's, and never survives the strict NMS
@pytest.mark.parametrize("seed,thr", [(0, 20), (1, 7), (2, 20), (3, 1), (4, 40), ("low_contrast", 0), ("spots", 0), ("spots", 1)])
def test_fast_matches_closed_form_definition(seed, thr):
    img = S.frame(96, 80, seed=seed + 11) if isinstance(seed, int) else OI.make(seed, 96, 80, 12)
    got = O.fast9_16(img, thr)
    exp = fast_definition(img, thr)
    assert len(got) > 0
    assert np.array_equal(got, exp)
    if thr == 0:  # the case is live: isolated corners of arc score 1 exist, and the oracle drops them
        A = _arc_scores(img)
        nb = np.max([np.roll(np.roll(A, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx], 0)
        lone = (A == 1) & (nb == 0)
        assert lone.sum() > 5 and not lone[got[:, 1], got[:, 0]].any()


def test_fast_on_roi_only_reads_roi():
    img = S.frame(200, 150, seed=5)
    roi = img[19:89, 19:89]
    a = O.fast9_16(roi, 20)
    b = O.fast9_16(np.ascontiguousarray(roi), 20)
    assert np.array_equal(a, b) and len(a) > 0


def test_resize_properties():
    const = np.full((50, 70), 93, np.uint8)
    assert (O.resize_linear(const, 58, 42) == 93).all()
    img = S.frame(120, 90, seed=3)
    assert np.array_equal(O.resize_linear(img, 120, 90), img)  # identity scale
    # exact fixed-point formula, restated in numpy
    dw, dh = 100, 75
    sx_scale, sy_scale = 1.0 / (dw / 120), 1.0 / (dh / 90)

    def coef(n, scale, lim):
        fx = ((np.arange(n) + 0.5) * scale - 0.5).astype(np.float32)
        s = np.floor(fx).astype(np.int32)
        f = fx - s.astype(np.float32)
        f[s < 0] = 0
        s[s < 0] = 0
        return s, f

    sx, fx = coef(dw, sx_scale, 120)
    sy, fy = coef(dh, sy_scale, 90)
    fx[sx >= 119] = 0
    sx = np.minimum(sx, 119)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int32)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int32)
    b1 = np.rint(fy * np.float32(2048)).astype(np.int32)
    b0 = np.rint((np.float32(1) - fy) * np.float32(2048)).astype(np.int32)
    I = img.astype(np.int32)
    sx1 = np.minimum(sx + 1, 119)
    H = I[:, sx] * a0 + I[:, sx1] * a1
    r0 = H[np.clip(sy, 0, 89)]
    r1 = H[np.clip(sy + 1, 0, 89)]
    exp = ((((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)
    assert np.array_equal(O.resize_linear(img, dw, dh), exp)


def test_blur_properties():
    const = np.full((40, 60), 201, np.uint8)
    assert (O.gaussian_blur7(const) == 201).all()
    img = S.frame(64, 48, seed=9)
    t = np.array([18, 34, 48, 56, 48, 34, 18], np.int64)
    p = np.pad(img.astype(np.int64), 3, mode="reflect")  # numpy 'reflect' == BORDER_REFLECT_101
    hpass = sum(t[k] * p[:, k:k + 64] for k in range(7))
    vpass = sum(t[k] * hpass[k:k + 48] for k in range(7))
    assert np.array_equal(O.gaussian_blur7(img), ((vpass + 32768) >> 16).astype(np.uint8))


def test_descriptor_bit_order_and_rotation_zero():
    img = S.frame(100, 100, seed=2)
    d = O.orb_descriptor(img, 50, 50, 0.0)
    # util::cos(0) = c1 != 1 and util::sin(0) = cos(pi/2) ~ 2.5e-4: rounding still lands on the integer pattern
    import re, pathlib
    pat = np.array([int(v) for v in re.findall(r"-?\d+", "".join(
        l for l in pathlib.Path(O._HERE / "orb_pattern_i8.inc").read_text().splitlines() if not l.startswith(("/*", " "))))],
        np.int32).reshape(256, 4)
    exp = np.zeros(32, np.uint8)
    for k in range(256):
        x0, y0, x1, y1 = pat[k]
        if img[50 + y0, 50 + x0] < img[50 + y1, 50 + x1]:
            exp[k // 8] |= 1 << (k % 8)
    assert np.array_equal(d, exp)


# ---- reference test/stella_vslam/feature/orb_extractor.cc:25-77: toy rectangle, keypoints near the corner
@pytest.mark.parametrize("size,rect,corner", [(600, (300, 300, 600, 600), (300, 300)), (1200, (0, 0, 1000, 1000), (1000, 1000))])
def test_toy_rectangle_keypoints_near_corner(size, rect, corner):
    img = np.full((size, size), 255, np.uint8)
    x0, y0, x1, y1 = rect
    img[y0:min(y1 + 1, size), x0:min(x1 + 1, size)] = 0  # cv::rectangle fills both corners inclusively
    kps, desc, counts = O.orb_extract(img, min_area=1000)
    assert len(kps) > 0 and desc.shape == (len(kps), 32) and desc.dtype == np.uint8
    sf = O.scale_tables(1.2, 8)[0]
    for kp in kps:
        tol = 2.0 * sf[kp["octave"]]
        assert abs(kp["x"] - corner[0]) <= tol and abs(kp["y"] - corner[1]) <= tol


# ---- reference :117-330: no keypoint inside the mask
def test_image_mask_excludes_keypoints():
    img = S.frame(960, 480, seed=21)
    h, w = img.shape
    mask = np.ones((h, w), np.uint8)
    mask[0:h // 4] = 0
    mask[3 * h // 4:h - 1] = 0
    kps, desc, _ = O.orb_extract(img, mask=mask, min_area=1000)
    assert len(kps) > 0 and len(desc) == len(kps)
    assert (kps["y"] >= h // 4).all() and (kps["y"] <= 3 * h // 4).all()
    mask = np.ones((h, w), np.uint8)
    mask[:, 0:w // 4] = 0
    mask[:, 3 * w // 4:w - 1] = 0
    kps, _, _ = O.orb_extract(img, mask=mask, min_area=1000)
    assert len(kps) > 0
    assert (kps["x"] >= w // 4).all() and (kps["x"] <= 3 * w // 4).all()


def test_extract_structure_640x480():
    img = S.frame()
    kps, desc, counts = O.orb_extract(img)
    assert 1800 <= len(kps) <= 2463  # selection-grid bound
    assert counts.sum() == len(kps)
    assert (np.diff(kps["octave"]) >= 0).all()  # level-major order
    assert (kps["class_id"] == -1).all()
    assert ((kps["angle"] >= 0) & (kps["angle"] <= 360)).all()
    sf = O.scale_tables(1.2, 8)[0]
    assert np.array_equal(kps["size"], np.floor(np.float32(31) * sf[kps["octave"]]).astype(np.float32))
    empty, _, _ = O.orb_extract(np.full((480, 640), 77, np.uint8))
    assert len(empty) == 0
