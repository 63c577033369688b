"""Problems and the CPU yardstick for image ingest (svgpu_ingest_*): colour to grey, rectification, true depth.

PARITY UNPINNED.  The reference pins OpenCV 4.7.0, which is not available to this project: the constants below restate OpenCV 4.x's 8-bit
paths from its published sources as remembered, not from a run against the library.  Until somebody compares against OpenCV itself, this
module IS the definition of what the device computes.

The yardstick restates, with integer arithmetic,
  (a) cv::cvtColor(..., COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) on 8U (util/image_converter.cc:8-39):
          grey = (R * 9798 + G * 19235 + B * 3735 + (1 << 14)) >> 15, alpha ignored, one channel passes through;
  (b) cv::remap(src, dst, map_x, map_y, INTER_LINEAR) with CV_32FC1 maps, BORDER_CONSTANT 0 (util/stereo_rectifier.cc:62-66):
          sx = rint(map_x * 32.0f) (fp32 product, half to even), ix = sx >> 5, fx = sx & 31, likewise y; the four weights
          (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx*fy, each times 32 (sum 32768); dst = (sum w * tap + (1 << 14)) >> 15 per channel;
          a tap outside the source counts as 0; a non-finite or huge entry gives 0 in every channel;
  (c) img.convertTo(img, CV_32F, 1.0 / depthmap_factor) (util/image_converter.cc:41-43): float(d) * float(1.0 / factor), one fp32 product.
The reference rectifies the image as read and converts to grey afterwards: `ingest` is remap per channel, then (a).
numpy only; shared by tests/test_ingest_restatement.py (CPU) and tests/test_gpu_ingest.py (GPU)."""
import numpy as np

GRAY, RGB, BGR = 0, 1, 2          # camera::color_order_t (camera/base.h:33-37)
DEPTH_U16, DEPTH_F32 = 1, 2       # svgpu_depth_type
F32 = np.float32
CR, CG, CB = 9798, 19235, 3735
FORMATS = {"GRAY": (1, GRAY), "RGB": (3, RGB), "BGR": (3, BGR), "RGBA": (4, RGB), "BGRA": (4, BGR)}
SIZES = [(640, 480), (752, 480), (1241, 376), (203, 157), (1920, 1080)]
MAP_CLASSES = ("identity", "fractional_shift", "plumb_bob", "quarter_outside", "non_finite")


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def to_gray(img, color_order):
    """(a).  img: (H, W) or (H, W, C) uint8 with C in {1, 3, 4}."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2 or img.shape[2] == 1:
        return img.reshape(img.shape[0], img.shape[1]).copy()
    if img.shape[2] not in (3, 4) or color_order not in (RGB, BGR):
        raise ValueError("colour order Gray with 3 or 4 channels, or an unsupported channel count")
    c = img.astype(np.int64)
    r, g, b = (c[..., 0], c[..., 1], c[..., 2]) if color_order == RGB else (c[..., 2], c[..., 1], c[..., 0])
    return ((r * CR + g * CG + b * CB + (1 << 14)) >> 15).astype(np.uint8)


def fixed_point(m):
    """sx = rint(m * 32.0f) of (b) -> (integer part, 5-bit fraction, usable).  Not usable: non-finite, or beyond int32."""
    with np.errstate(all="ignore"):
        v = np.rint(np.asarray(m, F32) * F32(32.0))     # fp32 product; np.rint rounds half to even
    ok = np.isfinite(v) & (np.abs(v) < F32(2.0 ** 30))
    s = np.where(ok, v, 0).astype(np.int64)
    return s >> 5, s & 31, ok


def weights(fx, fy):
    """The four bilinear weights of one fraction pair, in tap order (0,0) (1,0) (0,1) (1,1)."""
    return (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32


def remap(src, map_x, map_y):
    """(b).  src: (H, W) or (H, W, C) uint8; maps: (h, w) float32 -> (h, w[, C]) uint8."""
    src = np.asarray(src, np.uint8)
    squeeze = src.ndim == 2
    s = src.reshape(src.shape[0], src.shape[1], -1).astype(np.int64)
    H, W, _ = s.shape
    ix, fx, okx = fixed_point(map_x)
    iy, fy, oky = fixed_point(map_y)
    ok = okx & oky
    acc = np.zeros(ix.shape + (s.shape[2],), np.int64)
    for (dx, dy), w in zip(((0, 0), (1, 0), (0, 1), (1, 1)), weights(fx, fy)):
        x, y = ix + dx, iy + dy
        inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        tap = s[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        acc += np.where(inside, w, 0)[..., None] * tap
    out = ((acc + (1 << 14)) >> 15).astype(np.uint8)
    return out[..., 0] if squeeze else out


def ingest(raw, color_order, map_x=None, map_y=None):
    """What svgpu_ingest_gray computes: remap per channel (when maps are given), then grey."""
    if map_x is not None:
        raw = remap(raw, map_x, map_y)
    return to_gray(raw, color_order)


def true_depth(d, factor):
    """(c).  d: uint16 or float32."""
    d = np.asarray(d)
    assert d.dtype in (np.uint16, np.float32)
    return (d.astype(F32) * F32(1.0 / float(factor))).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- generators
def colour_image(gray_like, channels, seed):
    """An interleaved 8U image of `channels` channels whose channels differ (so that a swapped order or a leaking alpha shows)."""
    g = np.asarray(gray_like, np.uint8)
    if channels == 1:
        return g.copy()
    rng = np.random.default_rng(seed)
    h, w = g.shape
    out = np.empty((h, w, channels), np.uint8)
    out[..., 0] = g
    out[..., 1] = (g.astype(np.int32) * 3 // 4 + rng.integers(0, 64, (h, w))).astype(np.uint8)
    out[..., 2] = 255 - g // 2 - rng.integers(0, 32, (h, w)).astype(np.uint8)
    if channels == 4:
        out[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return out


def noise_image(w, h, channels, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels == 1 else (h, w, channels)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def strided(a, row_bytes):
    """A copy of the 2-D/3-D uint8 array `a` whose rows lie `row_bytes` apart (>= a row), as a view into a larger buffer filled with 0xA5."""
    a = np.ascontiguousarray(a)
    dense = a.shape[1] * (a.shape[2] if a.ndim == 3 else 1)
    assert row_bytes >= dense
    buf = np.full(a.shape[0] * row_bytes, 0xA5, np.uint8)
    v = np.lib.stride_tricks.as_strided(buf, shape=a.shape, strides=(row_bytes,) + a.strides[1:])
    v[...] = a
    return v


def _rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def plumb_bob_maps(w, h, seed=0, rot=(0.004, -0.006, 0.003), dist=(-0.2834, 0.0739, 0.00019, 1.76e-05, 0.0)):
    """Plausible rectification maps in the manner of cv::initUndistortRectifyMap (not equal to it): destination pixel -> inverse new camera
    -> inverse rotation -> plumb-bob distortion -> source camera, in fp64, rounded to fp32."""
    rng = np.random.default_rng(seed)
    fx = 0.72 * w * (1 + 0.01 * rng.standard_normal())
    fy = fx * (1 + 0.004 * rng.standard_normal())
    cx, cy = 0.5 * w + rng.uniform(-4, 4), 0.5 * h + rng.uniform(-4, 4)
    fxn, fyn, cxn, cyn = 0.97 * fx, 0.97 * fy, 0.5 * w, 0.5 * h
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    p = np.stack([(xx - cxn) / fxn, (yy - cyn) / fyn, np.ones_like(xx)], -1) @ _rot(np.asarray(rot, np.float64))   # rows times R = R^T applied
    x, y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return (fx * xd + cx).astype(F32), (fy * yd + cy).astype(F32)


def make_maps(kind, w, h, seed=0):
    """-> (map_x, map_y) float32 (h, w) of one of MAP_CLASSES."""
    yy, xx = np.mgrid[0:h, 0:w].astype(F32)
    rng = np.random.default_rng(seed)
    if kind == "identity":
        return xx.copy(), yy.copy()
    if kind == "fractional_shift":
        return (xx + F32(2.28125)).astype(F32), (yy - F32(1.59375)).astype(F32)
    if kind == "plumb_bob":
        return plumb_bob_maps(w, h, seed)
    mx, my = plumb_bob_maps(w, h, seed)
    if kind == "quarter_outside":     # a quarter of the entries point outside the source: beyond every border, and just across it
        pick = rng.random((h, w)) < 0.25
        far = rng.choice(np.array([-1e9, -3000.5, -1.0, -0.96875, w - 0.03125, w + 0.5, 5000.25, 1e9], np.float64), (h, w)).astype(F32)
        on_x = rng.random((h, w)) < 0.5
        mx = np.where(pick & on_x, far, mx).astype(F32)
        my = np.where(pick & ~on_x, np.where(far > 0, far - F32(w) + F32(h), far), my).astype(F32)
        return mx, my
    if kind == "non_finite":
        pick = rng.random((h, w)) < 0.1
        bad = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31], np.float64), (h, w)).astype(F32)
        on_x = rng.random((h, w)) < 0.5
        return np.where(pick & on_x, bad, mx).astype(F32), np.where(pick & ~on_x, bad, my).astype(F32)
    raise KeyError(kind)
