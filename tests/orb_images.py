"""Image classes that drive the parts of ORB extraction the natural-looking synthetic frames never reach: the min_fast_thr retry
of a FAST cell, the strict `> t` boundary of the threshold, threshold 0, saturated and binary content, and keypoints whose
intensity-centroid angle lands exactly on a quadrant edge of fastAtan2.  numpy only and deterministic; no oracle calls.
tests/test_orb_image_classes.py checks on the CPU oracle that each class does what its docstring claims."""
from __future__ import annotations

import numpy as np

from stella_vslam_amd import synthetic as S

CELL, BORDER = 64, 19  # FAST cell size and the patch-radius border of orb_extractor.cc (cells of level 0 start at x, y = 19 + 64 k)


def low_contrast(w: int = 640, h: int = 480, seed: int = 1) -> np.ndarray:
    """synthetic.frame // 8: values 0..31, most cells have no corner above ini_thr 20 and take the min_thr retry."""
    return S.frame(w, h, seed) // 8


def low_contrast_band(w: int = 640, h: int = 480, seed: int = 1) -> np.ndarray:
    """synthetic.frame // 4 + 100: a narrow band of values away from 0 and 255; contrast enough that the retry is rare."""
    return S.frame(w, h, seed) // 4 + 100


def half_low_contrast(w: int = 640, h: int = 480, seed: int = 1) -> np.ndarray:
    """Low contrast everywhere; the level-0 FAST cells of every other column of cells, alternating per row of cells (a checker of
    cells), also get 5x5 white squares, 16 px apart and kept 12 px inside the cell (out of the neighbours' 6-px overlap and
    3-px ring): cells that need the retry and cells that do not sit next to each other in one row of cells (k_fast walks
    consecutive cells)."""
    out = low_contrast(w, h, seed)
    for cy in range(BORDER, h - BORDER, CELL):
        for cx in range(BORDER, w - BORDER, CELL):
            if ((cx - BORDER) // CELL + (cy - BORDER) // CELL) % 2 == 0:
                continue
            for y in range(cy + 12, min(cy + CELL - 12, h - BORDER - 12), 16):
                for x in range(cx + 12, min(cx + CELL - 12, w - BORDER - 12), 16):
                    out[y:y + 5, x:x + 5] = 255
    return out


def checkerboard(w: int = 640, h: int = 480, d: int = 20, base: int = 100, square: int = 5) -> np.ndarray:
    """Two-level checkerboard, levels `base` and `base + d`: every FAST arc score on level 0 is exactly d (or 0), so d = t and
    d = t + 1 sit on the two sides of the strict `A > t` test.  The pyramid blends the two levels: only level 0 keeps d exactly."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // square) + (xx // square)) % 2 == 0, base, base + d).astype(np.uint8)


def saturated_checkerboard(w: int = 640, h: int = 480, square: int = 5) -> np.ndarray:
    """0 / 255 checkerboard: the largest possible arc scores (255) and differences at the ends of the uint8 range."""
    return checkerboard(w, h, 255, 0, square)


def binary_blobs(w: int = 640, h: int = 480, seed: int = 3) -> np.ndarray:
    """Random 0 / 255 blobs: a coarse random binary grid (cells of 3..9 px, irregular) upsampled by nearest neighbour."""
    rng = np.random.default_rng(seed)
    cx = np.cumsum(rng.integers(3, 10, w))
    cy = np.cumsum(rng.integers(3, 10, h))
    gx = np.searchsorted(cx, np.arange(w), side="right")
    gy = np.searchsorted(cy, np.arange(h), side="right")
    grid = rng.integers(0, 2, (h + 1, w + 1), dtype=np.uint8) * np.uint8(255)
    return np.ascontiguousarray(grid[gy][:, gx])


def noise(w: int = 640, h: int = 480, seed: int = 5) -> np.ndarray:
    """Uniform noise: a corner candidate at most pixels."""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def spots(w: int = 640, h: int = 480, seed: int = 6, base: int = 128) -> np.ndarray:
    """Flat `base` with isolated single-pixel spots of +-1 and +-2, 9 px apart (jittered): a spot of +-1 has arc score 1 and every
    pixel around it 0, a spot of +-2 has arc score 2.  Only thresholds 0 and 1 see them; at threshold 0 cv::FAST gives the +-1 spots
    the score A - 1 = 0, equal to a non-corner's, so its strict NMS drops every one of them."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), base, np.uint8)
    ys, xs = np.mgrid[4:h - 4:9, 4:w - 4:9]
    ys = ys + rng.integers(0, 2, ys.shape)
    xs = xs + rng.integers(0, 2, xs.shape)
    img[ys, xs] = (base + rng.choice(np.array([-2, -1, 1, 2]), ys.shape)).astype(np.uint8)
    return img


def symmetric_motifs(w: int = 640, h: int = 480, seed: int = 7) -> np.ndarray:
    """Bright motifs on a dark background, 40 px apart so that no 31-px orientation patch sees two of them, each mirror-symmetric
    about the row and / or the column of its apex pixel: right-angled wedges opening up, down, left or right (one moment is 0 by
    symmetry: intensity-centroid angle exactly 90 / 270 or 0 / 180) and 3x3 dots (both moments 0: fastAtan2(0, 0) = 0).  The
    brightness falls off with the distance from the apex, so the apex is the motif's single strongest corner (a two-level motif
    would give ties that the strict NMS drops)."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 30, np.uint8)
    yy, xx = np.mgrid[-8:9, -8:9]
    shade = (255 - 6 * np.rint(np.hypot(yy, xx))).astype(np.uint8)
    wedge = (yy >= 0) & (np.abs(xx) <= yy)  # apex at (0, 0), opening towards +y
    shapes = [wedge, wedge[::-1], wedge.T, wedge.T[:, ::-1], (np.abs(yy) <= 1) & (np.abs(xx) <= 1)]
    k = 0
    for cy in range(40, h - 40, 40):
        for cx in range(40, w - 40, 40):
            s = shapes[(k + int(rng.integers(0, 2))) % len(shapes)]
            k += 1
            img[cy - 8:cy + 9, cx - 8:cx + 9][s] = shade[s]
    return img


def probe(w: int, h: int, seed: int = 11) -> np.ndarray:
    """Low contrast on the left, texture on the right, noise in the bottom-right corner: retried and plain cells in one frame."""
    img = S.frame(w, h, seed)
    img[:, :w // 2] //= 8
    img[2 * h // 3:, 3 * w // 4:] = noise(w - 3 * w // 4, h - 2 * h // 3, seed)
    return img


def level0_cells(w: int, h: int):
    """The level-0 FAST cells of orb_extractor.cc:190-217 as (min_x, min_y, max_x, max_y): 64-px steps from the 19-px border, 6 px of
    overlap, clipped to the far border."""
    max_bx, max_by = w - BORDER, h - BORDER
    out = []
    for min_y in range(BORDER, max_by - 6, CELL):
        for min_x in range(BORDER, max_bx - 6, CELL):
            out.append((min_x, min_y, min(min_x + CELL + 6, max_bx), min(min_y + CELL + 6, max_by)))
    return out


def mask_retry_holes(img: np.ndarray, fast, ini_thr: int = 20, min_thr: int = 7, max_corners: int = 3):
    """A mask (1 = keep) with a zero hole over all the ini_thr corners of some level-0 cells, for the retry-before-mask order of
    orb_extractor.cc:228-256.  `fast(roi, t)` is cv::FAST with NMS returning (x, y, score) rows in ROI coordinates.  A cell is taken
    when it has 1..max_corners corners at ini_thr and min_thr corners outside their bounding box; its hole is that box grown by one
    pixel, which stays off the cell's own four corners (FAST never scores the 3-px rim).  Only cells of even row and column are
    taken, so no hole reaches the corners of another taken cell.  The reference finds the ini_thr corners, does not retry, and masks
    them all: the cell yields nothing; a kernel that masked before deciding on the retry would emit the min_thr corners.
    Returns (mask, taken cells as (min_x, min_y, max_x, max_y))."""
    h, w = img.shape
    mask = np.ones((h, w), np.uint8)
    taken = []
    for (x0, y0, x1, y1) in level0_cells(w, h):
        if ((x0 - BORDER) // CELL) % 2 or ((y0 - BORDER) // CELL) % 2:
            continue
        roi = img[y0:y1, x0:x1]
        hi = fast(roi, ini_thr)
        if not 1 <= len(hi) <= max_corners:
            continue
        bx0, by0 = hi[:, 0].min() - 1, hi[:, 1].min() - 1
        bx1, by1 = hi[:, 0].max() + 1, hi[:, 1].max() + 1
        lo = fast(roi, min_thr)
        outside = (lo[:, 0] < bx0) | (lo[:, 0] > bx1) | (lo[:, 1] < by0) | (lo[:, 1] > by1)
        if not outside.any():
            continue
        mask[y0 + by0:y0 + by1 + 1, x0 + bx0:x0 + bx1 + 1] = 0
        taken.append((x0, y0, x1, y1))
    return mask, taken


# every class at 640 x 480, for the single-frame parity sweeps
CLASSES = {
    "low_contrast": lambda: low_contrast(),
    "low_contrast_band": lambda: low_contrast_band(),
    "half_low_contrast": lambda: half_low_contrast(),
    "checker_d7": lambda: checkerboard(d=7),
    "checker_d8": lambda: checkerboard(d=8),
    "checker_d20": lambda: checkerboard(d=20),
    "checker_d21": lambda: checkerboard(d=21),
    "saturated_checker": lambda: saturated_checkerboard(),
    "binary_blobs": lambda: binary_blobs(),
    "noise": lambda: noise(),
    "spots": lambda: spots(),
    "symmetric_motifs": lambda: symmetric_motifs(),
}


def make(name: str, w: int, h: int, seed: int) -> np.ndarray:
    """One image of class `name` at any size (the random-geometry draws)."""
    if name.startswith("checker_d"):
        return checkerboard(w, h, int(name[len("checker_d"):]))
    f = {"low_contrast": low_contrast, "low_contrast_band": low_contrast_band, "half_low_contrast": half_low_contrast,
         "binary_blobs": binary_blobs, "noise": noise, "spots": spots, "symmetric_motifs": symmetric_motifs}.get(name)
    if f is not None:
        return f(w, h, seed)
    if name == "saturated_checker":
        return saturated_checkerboard(w, h)
    raise KeyError(name)
