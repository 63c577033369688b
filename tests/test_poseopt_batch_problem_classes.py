"""Every class of tests/poseopt_batch_problems.py has, under the CPU oracle (O.pose_optimize on the compacted arrays), the property that makes
it a class -- without exemption: a class that loses its property is repaired in the generator, not excused here.  Also: the C header
declares svgpu_pose_optimize_batch and the ctypes mirror sets its argument types."""
import pathlib
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import poseopt_batch_problems as PB

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _all():
    return [(call, p) for call, ps in PB.classes().items() for p in ps]


def _oracle(p, reset=False):
    s = PB.selected(p)
    return O.pose_optimize(s["pose_cw"], s["pos_w"], s["uvr"], s["inv_sigma_sq"], s["huber"], s["intr"], reset_flag_each_round=reset)


def _by_name(name):
    return next(p for _, p in _all() if p["name"] == name)


def test_every_class_is_present_once_and_states_its_property():
    names = [p["name"] for _, p in _all()]
    assert len(set(names)) == len(names)
    assert all(p["property"] for _, p in _all())
    for n in PB.SIZES:
        p = _by_name(f"size_{n}")
        assert len(p["pos_w"]) == n and p["select"] is None and p["active"]
    assert PB.SIZES == (0, 4, 5, 63, 64, 65, 511, 512, 513, 1200)
    for k in ("select_leaves_4", "select_leaves_5", "select_none", "select_every_second", "early_break", "inactive", "stereo_300", "equirect_300"):
        assert k in names


def test_batches_share_their_intrinsics_and_mix_skipped_with_optimised():
    C = PB.classes()
    for call, ps in C.items():
        b = PB.batch(ps)
        assert b["obs_off"][0] == 0 and b["obs_off"][-1] == len(b["pos_w"]) == len(b["select"])
    per = C["perspective"]
    skipped = [PB.is_skipped(p) for p in per]
    assert not skipped[0] and not skipped[-1] and any(skipped)
    assert max(range(len(per)), key=lambda k: len(per[k]["pos_w"])) not in (0, len(per) - 1)
    assert (C["stereo"][0]["uvr"][:, 2] >= 0).all() and C["stereo"][0]["intr"][4] > 0
    assert (C["perspective"][0]["uvr"][:, 2] < 0).all()
    assert np.array_equal(C["equirect"][0]["intr"][[0, 1, 4]], [0.0, 0.0, 0.0]) and C["equirect"][0]["intr"][2] > 0 and C["equirect"][0]["intr"][3] > 0


@pytest.mark.parametrize("reset", [False, True])
def test_sized_classes_optimise_from_five_entries_on(reset):
    for n in PB.SIZES:
        nv, pose, outl, st = _oracle(_by_name(f"size_{n}"), reset)
        if n < 5:
            assert nv == 0 and st[0] == 0 and np.array_equal(pose, _by_name(f"size_{n}")["pose_cw"])
        else:
            assert st[0] >= 1 and nv >= 5 and nv == n - outl.sum()
            assert not np.array_equal(pose, _by_name(f"size_{n}")["pose_cw"])


@pytest.mark.parametrize("reset", [False, True])
def test_select_classes(reset):
    p4, p5, p0, p2 = (_by_name(k) for k in ("select_leaves_4", "select_leaves_5", "select_none", "select_every_second"))
    assert p4["select"].sum() == 4 and len(p4["pos_w"]) > 5 and PB.is_skipped(p4)
    assert p5["select"].sum() == 5 and not PB.is_skipped(p5)
    nv, pose, outl, st = _oracle(p5, reset)
    assert st[0] >= 1 and nv == 5 and not np.array_equal(pose, p5["pose_cw"])  # the 5-entry class really optimises
    assert p0["select"].sum() == 0 and len(p0["pos_w"]) == 20 and PB.is_skipped(p0)
    assert len(p2["pos_w"]) == 130 and np.array_equal(np.flatnonzero(p2["select"]), np.arange(0, 130, 2))
    nv, pose, outl, st = _oracle(p2, reset)
    assert st[0] >= 1 and nv >= 5
    # the selected entries of the first wave do not fill it: entries of the second and third wave land in the first wave's range
    assert p2["select"][:64].sum() < 64 < p2["select"].sum()


@pytest.mark.parametrize("reset", [False, True])
def test_early_break_class_ends_below_five_valid_observations(reset):
    p = _by_name("early_break")
    assert p["select"] is None and len(p["pos_w"]) >= 5
    nv, pose, outl, st = _oracle(p, reset)
    assert nv < 5 and st[1] == len(p["pos_w"]) - nv
    assert 1 <= st[0] <= 10  # one round of at most num_each_iter iterations ran, then the break: three more would have followed
    # every class that optimises and is not this one runs all its rounds' classifications with five or more valid observations
    for _, q in _all():
        if q["name"] != "early_break" and not PB.is_skipped(q):
            assert _oracle(q, reset)[0] >= 5, q["name"]


def test_no_class_sits_on_a_decision_that_rounding_settles():
    for _, p in _all():
        assert PB.oracle_is_decided(p), p["name"]


def test_inactive_class_would_optimise_if_it_were_active():
    p = _by_name("inactive")
    assert not p["active"] and PB.is_skipped(p)
    nv, pose, outl, st = _oracle(p)
    assert st[0] >= 1 and nv >= 5


def test_stereo_and_equirectangular_classes_optimise():
    for name in ("stereo_300", "stereo_select", "equirect_300", "equirect_select"):
        p = _by_name(name)
        nv, pose, outl, st = _oracle(p)
        assert st[0] >= 1 and nv >= 5 and outl.sum() >= 1, name


def test_header_declares_the_symbol_and_the_mirror_sets_its_argtypes():
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    m = re.search(r"^int\s+svgpu_pose_optimize_batch\s*\(([^;]*)\);", hdr, flags=re.M)
    assert m is not None
    args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    assert len(args) == 19
    import ctypes as C
    from stella_vslam_amd import _lib
    fn = _lib.lib().svgpu_pose_optimize_batch
    vp, i32 = C.c_void_p, C.c_int
    assert fn.restype is C.c_int and fn.argtypes == [vp, i32] + [vp] * 9 + [i32] * 4 + [vp] * 4
