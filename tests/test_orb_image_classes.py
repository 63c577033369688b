"""Preconditions of tests/orb_images.py, on the CPU oracle: each image class drives the path of ORB extraction its docstring names
(the min_thr retry, both sides of the strict threshold test, exact quadrant angles, the retry-before-mask order).  Without these a
class could quietly become too easy and the GPU parity tests built on it would still pass."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import orb_images as OI


def _retried(k, ini=20):
    return k["response"] < ini  # cornerScore = A - 1 >= t: below ini_thr only from the min_thr pass


def test_low_contrast_drives_the_retry():
    k, _, _ = O.orb_extract(OI.low_contrast(640, 480, 1))
    assert len(k) > 500 and _retried(k).sum() >= 0.4 * len(k)  # 431 of 768


def test_low_contrast_band_rarely_retries():
    k, _, _ = O.orb_extract(OI.low_contrast_band(640, 480, 1))
    assert len(k) > 1000 and _retried(k).sum() <= 0.01 * len(k)


def test_half_low_contrast_mixes_retried_and_plain_cells():
    k, _, _ = O.orb_extract(OI.half_low_contrast(640, 480, 1))
    k0 = k[k["octave"] == 0]
    assert _retried(k0).sum() >= 30 and (~_retried(k0)).sum() >= 100


@pytest.mark.parametrize("d,retried", [(8, True), (20, True), (21, False)])
def test_checkerboard_threshold_boundaries(d, retried):
    """Level 0 of a two-level checkerboard has arc scores of exactly d: d = min_thr + 1 and d = ini_thr take the retry (A > t fails at
    ini_thr), d = ini_thr + 1 does not."""
    k, _, counts = O.orb_extract(OI.checkerboard(640, 480, d))
    k0 = k[k["octave"] == 0]
    assert counts[0] == len(k0) == 86
    assert (k0["response"] == d - 1).all()
    assert _retried(k0).all() if retried else not _retried(k0).any()


def test_checkerboard_at_min_thr_has_no_corner_at_all():
    k, _, counts = O.orb_extract(OI.checkerboard(640, 480, 7))
    assert len(k) == 0 and not counts.any()


@pytest.mark.parametrize("name", ["symmetric_motifs", "checker_d20", "saturated_checker"])
def test_quadrant_angles_are_exact(name):
    """fastAtan2 at m10 = 0 or m01 = 0 (and both): angles of exactly 0, 90, 180 and 270 degrees."""
    k, _, _ = O.orb_extract(OI.CLASSES[name]())
    for a in (0.0, 90.0, 180.0, 270.0):
        assert (k["angle"] == np.float32(a)).sum() >= 15, (name, a)
    if name == "symmetric_motifs":
        assert ((k["octave"] == 0) & np.isin(k["angle"], [0.0, 90.0, 180.0, 270.0])).sum() >= 100


def test_saturated_and_binary_classes_reach_the_largest_scores():
    for img in (OI.saturated_checkerboard(), OI.binary_blobs()):
        k, _, _ = O.orb_extract(img)
        assert len(k) > 1500 and k["response"].max() == 254  # arc score 255
    assert set(np.unique(OI.binary_blobs())) == {0, 255}


def test_spots_only_at_thresholds_0_and_1():
    img = OI.spots()
    assert len(O.orb_extract(img)[0]) == 0
    k0 = O.orb_extract(img, ini_thr=0, min_thr=0)[0]
    k1 = O.orb_extract(img, ini_thr=1, min_thr=1)[0]
    assert len(k0) > 100 and len(k1) > 100
    l0 = O.fast9_16(img, 0)
    assert len(l0) > 0 and (l0[:, 2] == 1).all()  # +-2 spots only: every +-1 spot (score 0 at threshold 0) lost the strict NMS


def test_mask_retry_holes_cover_only_first_pass_corners():
    img = OI.low_contrast(640, 480, 1)
    mask, cells = OI.mask_retry_holes(img, O.fast9_16)
    assert len(cells) >= 3
    k, _, _ = O.orb_extract(img, mask=mask)
    kf, _, _ = O.orb_extract(img)
    hits = 0
    for (x0, y0, x1, y1) in cells:
        for (x, y) in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):  # the cell is not skipped
            assert mask[min(y, 479), min(x, 639)] == 1
        roi, m = img[y0:y1, x0:x1], mask[y0:y1, x0:x1]
        hi, lo = O.fast9_16(roi, 20), O.fast9_16(roi, 7)
        assert (m[hi[:, 1], hi[:, 0]] == 0).all() and (m[lo[:, 1], lo[:, 0]] == 1).any()

        def inside(kk):
            return ((kk["octave"] == 0) & (kk["x"] >= x0 + 9) & (kk["x"] < x1 - 9) & (kk["y"] >= y0 + 9) & (kk["y"] < y1 - 9)).sum()
        assert inside(k) == 0
        hits += inside(kf)
    assert hits > 0  # without the mask those cells do emit keypoints


@pytest.mark.parametrize("w,h", [(621, 429), (622, 430), (677, 485)])
def test_probe_sizes_have_partial_edge_cells_and_retried_cells(w, h):
    assert (w - 38) % 64 in (7, 8, 63) and (h - 38) % 64 in (7, 8, 63)
    k, _, _ = O.orb_extract(OI.probe(w, h))
    assert _retried(k).sum() > 20 and (~_retried(k)).sum() > 500


def test_classes_are_deterministic():
    for name, f in OI.CLASSES.items():
        a, b = f(), f()
        assert a.dtype == np.uint8 and a.shape == (480, 640) and np.array_equal(a, b), name
        assert np.array_equal(OI.make(name, 640, 480, 1), OI.make(name, 640, 480, 1)), name
