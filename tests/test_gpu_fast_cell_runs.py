"""k_fast with several cells per workgroup: what it keeps from one cell to the next (the level record, the source base and pitch, the
band masks and staging predicates of the cell's size, the cleared arc-score array) against runs of consecutive cells in which those
things change.  Small images whose cell tables put into ONE workgroup of four cells: a level change; a last-column cell (w < 70)
followed by a full one; a last-row cell (h < 70); a cell without a corner at ini_thr (it takes the min_thr retry) between two textured
ones; and a cell that the mask removes.  Keypoints, responses and descriptors against the CPU oracle; the cell table is printed and
each of the cases is asserted to occur."""
import contextlib
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import orb_images as OI
from tests.test_gpu_orb_edges import _batch, _check_batch

pytestmark = pytest.mark.gpu

CPW, NL, SF, INI, MIN = 4, 8, 1.2, 20, 7
BORDER, CELL, OVERLAP = 19, 64, 6


@contextlib.contextmanager
def _cells_per_workgroup(n):
    """SVGPU_FAST_CPW is read at every extract call; restored afterwards."""
    saved = os.environ.get("SVGPU_FAST_CPW")
    os.environ["SVGPU_FAST_CPW"] = str(n)
    try:
        yield
    finally:
        os.environ.pop("SVGPU_FAST_CPW", None)
        if saved is not None:
            os.environ["SVGPU_FAST_CPW"] = saved


def cell_table(w, h):
    """The FAST cells of orb_extractor.cc:179-217 in the order k_fast walks them: (level, min_x, min_y, w, h)."""
    cells = []
    for l, (lw, lh) in enumerate(O.level_sizes(w, h, SF, NL)):
        if lw <= 2 * BORDER or lh <= 2 * BORDER:
            continue
        max_bx, max_by = lw - BORDER, lh - BORDER
        for i in range((max_by - BORDER) // CELL + 1):
            min_y = BORDER + i * CELL
            if max_by - OVERLAP <= min_y:
                continue
            for j in range((max_bx - BORDER) // CELL + 1):
                min_x = BORDER + j * CELL
                if max_bx - OVERLAP <= min_x:
                    continue
                cells.append((l, min_x, min_y, min(min_x + CELL + OVERLAP, max_bx) - min_x, min(min_y + CELL + OVERLAP, max_by) - min_y))
    return cells


def _mask_removes(cell, mask, scales):
    """orb_extractor.cc:168-170, :219-225: a cell is skipped when one of its four corners, scaled to level 0, is masked."""
    l, x, y, cw, ch = cell
    mh, mw = mask.shape

    def masked(yy, xx):
        my = min(int(np.float32(yy) * scales[l]), mh - 1)
        mx = min(int(np.float32(xx) * scales[l]), mw - 1)
        return mask[my, mx] == 0
    return masked(y, x) or masked(y + ch, x) or masked(y, x + cw) or masked(y + ch, x + cw)


def _scene(w, h):
    """Noise (a corner candidate at most pixels) with the second cell of the first workgroup flattened to low contrast: nothing in
    it reaches ini_thr, the retry at min_thr finds corners.  The mask takes out the third cell of the second workgroup."""
    cells = cell_table(w, h)
    img = OI.noise(w, h, 9)
    l, x, y, cw, ch = cells[1]
    assert l == 0
    img[y:y + ch, x:x + cw] //= 16
    mask = np.ones((h, w), np.uint8)
    l, x, y, cw, ch = cells[CPW + 2]
    scale = O.scale_tables(SF, NL)[0][l]
    mask[min(int(np.float32(y) * scale), h - 1), min(int(np.float32(x) * scale), w - 1)] = 0  # its first corner, in level-0 coordinates
    return img, mask, cells


@pytest.mark.parametrize("w,h", [(203, 157), (331, 250)])
def test_cell_runs_of_one_workgroup(w, h):
    from stella_vslam_amd import feature as F
    img, mask, cells = _scene(w, h)
    scales = O.scale_tables(SF, NL)[0]
    groups = [cells[i:i + CPW] for i in range(0, len(cells), CPW)]
    removed = [_mask_removes(c, mask, scales) for c in cells]
    print(f"{w} x {h}: {len(cells)} cells, {CPW} per workgroup")
    for gi, g in enumerate(groups):
        print(f"  workgroup {gi}: " + "  ".join(f"L{c[0]} ({c[1]},{c[2]}) {c[3]}x{c[4]}{' masked' if removed[gi * CPW + k] else ''}" for k, c in enumerate(g)))
    pairs = [(g[k], g[k + 1]) for g in groups for k in range(len(g) - 1)]
    assert any(a[0] != b[0] for a, b in pairs), "no level change inside a workgroup"
    assert any(a[3] < 70 and b[3] == 70 and a[0] == b[0] for a, b in pairs), "no last-column cell followed by a full one"
    assert any(c[4] < 70 and k > 0 for g in groups for k, c in enumerate(g)), "no last-row cell behind another cell"
    assert any(a[4] == 70 and b[4] < 70 and a[0] == b[0] for a, b in pairs), "no change of the cell height inside a workgroup"
    # the low-contrast cell: second of its workgroup, full size, no corner at ini_thr, some at min_thr; textured neighbours on both sides
    l, x, y, cw, ch = cells[1]
    assert (cw, ch) == (70, 70) and cells[0][0] == cells[2][0] == 0
    assert len(O.fast9_16(img[y:y + ch, x:x + cw], INI)) == 0 and len(O.fast9_16(img[y:y + ch, x:x + cw], MIN)) > 0
    for (l2, x2, y2, cw2, ch2) in (cells[0], cells[2]):
        assert len(O.fast9_16(img[y2:y2 + ch2, x2:x2 + cw2], INI)) > 0
    # the mask removes the third cell of the second workgroup and leaves that workgroup's other cells
    assert removed[CPW + 2] and not removed[CPW + 1] and not removed[CPW + 3]

    with _cells_per_workgroup(CPW):
        frames = np.stack([img, OI.noise(w, h, 4), img])
        plain = _batch(F, frames, "bands", ini=INI, mn=MIN, download=False)
        _check_batch(plain, frames, ini=INI, mn=MIN, what=("plain", w, h))
        masks = np.stack([mask, np.ones_like(mask), mask])
        res = _batch(F, frames, "bands", masks=masks, ini=INI, mn=MIN, mpad=3, moff=1, download=False)
        _check_batch(res, frames, masks, ini=INI, mn=MIN, what=("masked", w, h))
    assert (plain[0][0]["response"] < INI).any()            # the retry pass contributed
    assert len(res[0][0]) < len(plain[0][0])                # the mask removed something
    assert len(plain[0][0]) > 50


@pytest.mark.parametrize("cpw", [1, 2, 3, 5, 64])
def test_any_cells_per_workgroup_gives_the_same_keypoints(cpw):
    """The results do not depend on how the cells are dealt to the workgroups (runs that start and end anywhere in the table)."""
    from stella_vslam_amd import feature as F
    w, h = 203, 157
    img, mask, _ = _scene(w, h)
    frames = np.stack([img, img])
    masks = np.stack([np.ones_like(mask), mask])
    with _cells_per_workgroup(cpw):
        res = _batch(F, frames, "bands", masks=masks, ini=INI, mn=MIN, download=False)
    _check_batch(res, frames, masks, ini=INI, mn=MIN, what=("cpw", cpw))
