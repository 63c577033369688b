"""The prologues of k_pyramid_lds and k_describe_bands against the CPU oracle, bit for bit (stored pyramid levels, level counts, keypoints,
descriptors), through the batch entry point.  k_pyramid_lds keeps every level's scalars in LDS and fetches a thread's column record one
level ahead; k_describe_bands issues its row copy before it knows whether the band has keypoints and drains it when it has none.  The
cases are the ones in which that order can go wrong: bands without keypoints beside full ones, a capacity that cuts a band's run, 1 / 2 / 8
levels (no prefetch, one, the whole chain), level geometries that change sharply, levels with one row per thread, an unaligned caller image,
rows wider than 1 KB.

Which kernels ran: the profile classes of svgpu_profile_read_class ("k_resize", "k_describe") name the stage, not the variant, so the test
asks the planner itself -- tests/orb_prologue_plan.cpp is built with g++ against orb_plan.h and prints orb_launch_plan's decision for the
configuration (with SVGPU_DESCRIBE_BANDS set, as the batch helper sets it), the band table and the thread geometry of the pyramid."""
import ctypes as C
import functools
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as O
from stella_vslam_amd import synthetic as S
from tests.host_check import FLAGS, ROOT
from tests.test_gpu_orb_edges import KP_FIELDS, _describe, _oracle

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _plan_exe():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/orb_prologue_plan.cpp")
    exe = tempfile.mkdtemp(prefix="orb_prologue_plan_") + "/orb_prologue_plan"
    subprocess.check_call([cxx, *FLAGS, "-ffp-contract=off", "-I", str(ROOT / "stella_vslam_amd" / "csrc"), "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "orb_prologue_plan.cpp"), "-o", exe])
    return exe


@functools.lru_cache(maxsize=None)
def _plan(w, h, batch, sf, nl, ini=20, mn=7, area=800, aligned=True):
    """The planner's decisions for one configuration (tests/orb_prologue_plan.cpp); bands in emission order (by first cell)."""
    out = subprocess.run([_plan_exe(), *map(str, (w, h, batch, sf, nl, ini, mn, area, int(aligned)))], capture_output=True, text=True, check=True).stdout
    lines = [ln.split() for ln in out.splitlines()]
    head = [ln for ln in lines if ln[0] == "plan"][0]
    keys = ("pyramid_lds", "describe_bands", "pyr_bands", "pyr_lds_bytes", "pyr_cpr0", "desc_max_cpr", "rc1", "rc_more")
    plan = dict(zip(keys, map(int, head[1:])))
    plan["bands"] = sorted(tuple(map(int, ln[1:])) for ln in lines if ln[0] == "band")  # (cell0, cell1, level, y0, y1)
    return plan


def _assert_lds_kernels(plan):
    assert plan["pyramid_lds"] == 1 and plan["pyr_lds_bytes"] > 0, plan  # k_pyramid_lds, not k_pyramid
    assert plan["describe_bands"] == 1 and plan["bands"], plan              # k_describe_bands, not k_describe


def _band_counts(plan, ko, sf):
    """Keypoints of the oracle per describe band, in emission order (a band's keypoints are one contiguous run of it)."""
    scale = np.float32(sf) ** np.arange(16, dtype=np.float32)
    lev_y = np.where(ko["octave"] == 0, ko["y"], np.rint(ko["y"] / scale[ko["octave"]])).astype(int)
    counts = [int(((ko["octave"] == lv) & (lev_y >= y0) & (lev_y <= y1)).sum()) for (_, _, lv, y0, y1) in plan["bands"]]
    assert sum(counts) == len(ko), (sum(counts), len(ko))  # the bands partition the keypoints
    return counts


def _run(F, frames, sf=1.2, nl=8, pad=0, off=0, cap=None):
    """svgpu_orb_extract_batch_device with k_describe_bands forced; per frame (keypoints, descriptors, counts, pyramid levels)."""
    import torch
    from stella_vslam_amd._lib import lib
    L = lib()
    B, h, w = frames.shape
    with _describe("bands"):
        ctx = F.Context(0)
        ctx.check(L.svgpu_orb_configure(ctx.handle, w, h, B, C.c_float(sf), nl, 20, 7, C.c_uint(800)), "cfg")
        full = max(L.svgpu_orb_max_keypoints(ctx.handle), 1)
        cap = cap or full
        stride = w + pad
        fstride = h * stride + (pad & 1)
        host = np.zeros(off + B * fstride + 64, np.uint8)
        for b in range(B):
            host[off + b * fstride: off + b * fstride + h * stride].reshape(h, stride)[:, :w] = frames[b]
        img = torch.from_numpy(host).cuda()
        kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
        desc = torch.full((B * cap * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(B * (1 + nl), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.check(L.svgpu_orb_extract_batch_device(ctx.handle, C.c_void_p(img.data_ptr() + off), B, C.c_size_t(fstride), stride, None, C.c_size_t(0), 0,
                                                   C.c_void_p(kps.data_ptr()), C.c_void_p(desc.data_ptr()), cap, C.c_void_p(counts.data_ptr()), None), "extract")
        ctx.synchronize()
    kk = kps.cpu().numpy().view(O.KEYPOINT_DTYPE).reshape(B, cap)
    dd = desc.cpu().numpy().reshape(B, cap, 32)
    cc = counts.cpu().numpy().reshape(B, 1 + nl)
    out = []
    for b in range(B):
        pyr = []
        for l in range(nl):
            lw, lh = C.c_int(), C.c_int()
            ctx.check(L.svgpu_orb_level_size(ctx.handle, l, C.byref(lw), C.byref(lh)), "level_size")
            a = np.zeros((lh.value, lw.value), np.uint8)
            ctx.check(L.svgpu_orb_pyramid_download(ctx.handle, b, l, a.ctypes.data_as(C.c_void_p), lw.value), "pyr")
            pyr.append(a)
        out.append((kk[b], dd[b], cc[b], pyr))
    return out


def _check(res, frames, sf, nl, what, cap=None):
    """Every frame against the oracle; with `cap` the first `cap` keypoints of the emission order and nothing written behind them.
    Returns the oracle's keypoints per frame."""
    kos = []
    for b, (k, d, c, pyr) in enumerate(res):
        ko, do, counts, opyr = _oracle(frames[b], None, sf, nl)
        assert len(pyr) == len(opyr) == nl
        for l, (a, o) in enumerate(zip(pyr, opyr)):
            assert a.shape == o.shape and np.array_equal(a, o), (what, b, "pyramid level", l)
        assert np.array_equal(c[1:], counts) and c[0] == len(ko), (what, b, c, counts)
        n = len(ko) if cap is None else min(cap, len(ko))
        for f in KP_FIELDS:
            assert np.array_equal(k[:n][f], ko[:n][f]), (what, b, f)
        assert np.array_equal(d[:n], do[:n]), (what, b)
        assert (d[n:] == 0xAB).all(), (what, b, "descriptor written behind the run")
        kos.append(ko)
    return kos


@pytest.fixture(scope="module")
def F():
    from stella_vslam_amd import feature
    return feature


W, H = 320, 240


def _half(seed):
    img = S.frame(W, H, seed).copy()
    img[H // 2:] = 90
    return img


# ------------------------------------------------------------------------------------------------------------ 1. empty bands beside full ones
def test_empty_bands_beside_full_ones(F):
    """Upper half textured, lower half constant: the bands of the lower half have no keypoints and return behind their row copy, next to
    bands that describe; one frame of the batch is constant (every band empty), one textured all over (no band of level 0 empty)."""
    frames = np.stack([_half(31), np.full((H, W), 90, np.uint8), S.frame(W, H, 32), _half(33)])
    plan = _plan(W, H, len(frames), 1.2, 8)
    _assert_lds_kernels(plan)
    kos = _check(_run(F, frames), frames, 1.2, 8, "empty bands")
    per_frame = [_band_counts(plan, ko, 1.2) for ko in kos]
    for b in (0, 3):
        assert min(per_frame[b]) == 0 and max(per_frame[b]) > 20, per_frame[b]  # empty bands beside full ones
        lv0 = [n for n, bd in zip(per_frame[b], plan["bands"]) if bd[2] == 0]
        assert 0 in lv0 and max(lv0) > 20, lv0
    assert len(kos[1]) == 0 and sum(per_frame[1]) == 0
    assert all(n > 0 for n, bd in zip(per_frame[2], plan["bands"]) if bd[2] == 0), per_frame[2]


# ------------------------------------------------------------------------------------------------------------ 2. capacity cuts a band's run
def test_capacity_cuts_a_run_inside_a_band(F):
    """Fewer slots than keypoints: the band the capacity falls into describes the head of its run (a positive, shortened count), every band
    behind it finds none left (count <= 0) although its cells hold keypoints."""
    frames = S.frame_sequence(2, W, H, seed=41)
    plan = _plan(W, H, len(frames), 1.2, 8)
    _assert_lds_kernels(plan)
    runs = []
    for b in range(len(frames)):
        ko = _oracle(frames[b], None, 1.2, 8)[0]
        cnt = _band_counts(plan, ko, 1.2)
        runs.append((np.concatenate([[0], np.cumsum(cnt)]), cnt, len(ko)))
    # a capacity strictly inside the run of a band of frame 0 that has at least two keypoints, with non-empty bands behind it
    start, cnt, total = runs[0]
    i = next(i for i in range(len(cnt)) if cnt[i] >= 2 and start[i] > total // 3)
    cap = int(start[i]) + cnt[i] // 2
    for start, cnt, total in runs:
        assert total > cap  # counts > cap in every frame
        cut = [j for j in range(len(cnt)) if start[j] < cap < start[j] + cnt[j]]
        gone = [j for j in range(len(cnt)) if cnt[j] > 0 and start[j] >= cap]
        assert gone, (cap, list(start))
        if start is runs[0][0]:
            assert cut == [i]
    _check(_run(F, frames, cap=cap), frames, 1.2, 8, "capacity", cap=cap)


# ------------------------------------------------------------------------------------------------------------ 3. level counts and geometries
@pytest.mark.parametrize("w,h,sf,nl,need", [
    (W, H, 1.2, 1, "one level"),     # nothing to resize: the planner gives k_pyramid_lds no LDS and launches the (then empty) k_pyramid
    (W, H, 1.2, 2, "two levels"),    # one record fetched in the prologue, none in the loop
    (640, 480, 1.2, 8, "rc_more"),   # the whole chain, threads that walk several rows
    (W, H, 2.0, 4, "rc1"),           # 320 -> 160 -> 80 -> 40 px: groups per row, chunks and rows per chunk change sharply from level to level
    (131, 100, 1.2, 8, "rc1"),       # deep levels of a few rows: one row per thread, most threads without rows
])
def test_level_counts_and_thread_geometries(F, w, h, sf, nl, need):
    frames = S.frame_sequence(2, w, h, seed=w + nl)
    plan = _plan(w, h, len(frames), sf, nl)
    if nl == 1:
        assert plan["pyramid_lds"] == 0 and plan["describe_bands"] == 1, plan
    else:
        _assert_lds_kernels(plan)
    if need == "rc1":
        assert plan["rc1"] > 0, plan
    elif need == "rc_more":
        assert plan["rc_more"] > 0 and plan["rc1"] > 0, plan  # both kinds of level in one workgroup's life
    else:
        assert (plan["rc1"] + plan["rc_more"] == 0) == (nl == 1), plan
    kos = _check(_run(F, frames, sf, nl), frames, sf, nl, (w, h, sf, nl))
    assert min(len(ko) for ko in kos) > 20


# ------------------------------------------------------------------------------------------------------------ 4. unaligned caller image
def test_unaligned_caller_image(F):
    """Base address 1 byte past alignment and an odd row pitch: level 0 of the pyramid is staged byte by byte (no LDS-DMA), the column
    records are fetched ahead all the same; the 324-byte pitch of the second run takes the dword path."""
    frames = S.frame_sequence(2, W + 3, H + 3, seed=51)  # 323 x 243
    plan = _plan(W + 3, H + 3, len(frames), 1.2, 8, aligned=False)
    _assert_lds_kernels(plan)
    for pad, off in ((0, 1), (1, 0)):
        kos = _check(_run(F, frames, pad=pad, off=off), frames, 1.2, 8, ("unaligned", pad, off))
        assert min(len(ko) for ko in kos) > 50


# ------------------------------------------------------------------------------------------------------------ 5. rows wider than 1 KB
def test_rows_wider_than_1kb(F):
    """1296 x 80 px, two levels: a staged level-0 row of k_pyramid_lds is 81 sixteen-byte pieces and a band row of k_describe_bands 82 -- more
    than the 64 lanes of one copy instruction, so both kernels stage with db_stage_rows_wide; the planner still chooses the LDS forms here."""
    w, h, nl = 1296, 80, 2
    frames = S.frame_sequence(2, w, h, seed=61)
    plan = _plan(w, h, len(frames), 1.2, nl)
    _assert_lds_kernels(plan)
    assert plan["pyr_cpr0"] > 64 and plan["desc_max_cpr"] > 64, plan
    kos = _check(_run(F, frames, 1.2, nl), frames, 1.2, nl, "wide")
    assert min(len(ko) for ko in kos) > 50
