"""Python mirror of image ingest over the C ABI (include/svgpu.h svgpu_ingest_*): what system::create_*_frame does to an image before the
extractor sees it -- util::convert_to_grayscale, util::stereo_rectifier::rectify and util::convert_to_true_depth
(util/image_converter.cc:8-43, util/stereo_rectifier.cc:62-66) -- on the device, in OpenCV's 8-bit fixed-point arithmetic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, ptr as _p
from .feature import Context

COLOR_GRAY, COLOR_RGB, COLOR_BGR = 0, 1, 2      # camera::color_order_t
DEPTH_NONE, DEPTH_U16, DEPTH_F32 = 0, 1, 2
_ORDERS = {"gray": COLOR_GRAY, "rgb": COLOR_RGB, "bgr": COLOR_BGR}


class Ingest:
    """svgpu_ingest: the raw frame format of one camera and, for a rectified camera, its compiled maps.

    `color_order`: "Gray" | "RGB" | "BGR" (or the enum value); `map_x` / `map_y`: float32 (height, width) as the reference's
    stereo_rectifier holds them, or both None."""

    def __init__(self, ctx: Context, width: int, height: int, channels: int, color_order, map_x: np.ndarray | None = None, map_y: np.ndarray | None = None):
        self.ctx, self.width, self.height, self.channels = ctx, int(width), int(height), int(channels)
        self.color_order = _ORDERS[color_order.lower()] if isinstance(color_order, str) else int(color_order)
        self._h = C.c_void_p()
        mx = my = None
        stride = 0
        if map_x is not None or map_y is not None:
            if map_x is None or map_y is None:
                raise ValueError("map_x and map_y go together")
            mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
            if mx.shape != (self.height, self.width) or my.shape != mx.shape:
                raise ValueError("the maps must have the image's size")
            stride = mx.strides[0]
        ctx.check(lib().svgpu_ingest_create(ctx.handle, self.width, self.height, self.channels, self.color_order, _p(mx), _p(my), stride, C.byref(self._h)),
                  "svgpu_ingest_create")

    def _raw(self, img):
        im = np.asarray(img)
        if im.dtype != np.uint8 or im.ndim not in (2, 3) or im.shape[0] != self.height or im.shape[1] != self.width \
                or (im.shape[2] if im.ndim == 3 else 1) != self.channels:
            raise TypeError("frame must be uint8 (height, width[, channels]) in the ingest's format")
        if im.strides[-1] != 1 or (im.ndim == 3 and im.strides[1] != self.channels):
            im = np.ascontiguousarray(im)
        return im

    def gray(self, img: np.ndarray, out: np.ndarray | None = None, ctx: Context | None = None) -> np.ndarray:
        """One frame, host in / host out (svgpu_ingest_gray).  `img` may have padded rows; so may `out` (uint8 (height, width))."""
        c = ctx or self.ctx
        im = self._raw(img)
        if out is None:
            out = np.empty((self.height, self.width), np.uint8)
        assert out.dtype == np.uint8 and out.shape == (self.height, self.width) and out.strides[1] == 1
        c.check(lib().svgpu_ingest_gray(c.handle, self._h, _p(im), im.strides[0], _p(out), out.strides[0]), "svgpu_ingest_gray")
        return out

    def gray_batch_device(self, src_dev: int, batch: int, src_frame_stride: int, src_row_stride: int, dst_dev: int, dst_frame_stride: int, dst_row_stride: int,
                          stream: int | None = None, ctx: Context | None = None):
        """`batch` raw frames in HBM -> grey frames in HBM, asynchronous (svgpu_ingest_gray_batch_device); pointers as integers
        (torch: tensor.data_ptr()).  The output layout is svgpu_orb_extract_batch_device's imgs_dev."""
        c = ctx or self.ctx
        c.check(lib().svgpu_ingest_gray_batch_device(c.handle, self._h, src_dev, batch, src_frame_stride, src_row_stride, dst_dev,
                                                     dst_frame_stride, dst_row_stride, stream or None), "svgpu_ingest_gray_batch_device")

    def close(self):
        if self._h:
            lib().svgpu_ingest_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def depth_type_of(dtype) -> int:
    dt = np.dtype(dtype)
    if dt == np.uint16:
        return DEPTH_U16
    if dt == np.float32:
        return DEPTH_F32
    raise TypeError("depth maps are uint16 or float32")


def gray(ctx: Context, img: np.ndarray, color_order, map_x=None, map_y=None) -> np.ndarray:
    """convert_to_grayscale (and rectify, with maps) of one frame: a throw-away Ingest."""
    im = np.asarray(img)
    g = Ingest(ctx, im.shape[1], im.shape[0], im.shape[2] if im.ndim == 3 else 1, color_order, map_x, map_y)
    try:
        return g.gray(im)
    finally:
        g.close()


def gray_batch_device(ing: Ingest, *args, **kw):
    return ing.gray_batch_device(*args, **kw)


def depth(ctx: Context, img: np.ndarray, depthmap_factor: float) -> np.ndarray:
    """convert_to_true_depth: uint16 / float32 (height, width) -> float32 metres (svgpu_ingest_depth)."""
    d = np.asarray(img)
    t = depth_type_of(d.dtype)
    if d.ndim != 2:
        raise TypeError("depth map must be 2-D")
    if d.strides[1] != d.itemsize:
        d = np.ascontiguousarray(d)
    out = np.empty(d.shape, np.float32)
    ctx.check(lib().svgpu_ingest_depth(ctx.handle, _p(d), t, d.strides[0], d.shape[1], d.shape[0], float(depthmap_factor), _p(out), out.strides[0]),
              "svgpu_ingest_depth")
    return out


def depth_device(ctx: Context, src_dev: int, src_type: int, src_stride: int, width: int, height: int, depthmap_factor: float, dst_dev: int, dst_stride: int,
                 stream: int | None = None):
    ctx.check(lib().svgpu_ingest_depth_device(ctx.handle, src_dev, src_type, src_stride, width, height, float(depthmap_factor), dst_dev,
                                              dst_stride, stream or None), "svgpu_ingest_depth_device")
