"""The problem classes of tests/loop_sim3_problems.py are what they claim to be, shown on the CPU by the numpy restatement of the scale alone
(module/loop_detector.cc:540-573): the number of kept ratios per candidate, the candidates that end without a scale, and where the planted
boundary pairs sit."""
import pathlib
import re

import numpy as np
import pytest

from tests import loop_sim3_problems as LP

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def problems():
    return LP.classes()


@pytest.fixture(scope="module")
def scale_problems():
    return LP.scale_classes()


def test_every_class_keeps_the_ratios_its_knobs_plant(problems):
    for name, p in problems.items():
        for c in range(p["num_candidates"]):
            s, kept, idx = LP.scale_restatement(p, c)
            assert len(kept) == LP.planted_kept(p, c), (name, c)
            assert (kept > 0).all() and np.isfinite(kept).all()
            if len(kept):
                assert abs(float(s) - 1.05) < 2e-3 or name == "stereo_fix_scale", (name, c, s)
                assert (p["prior_state"][c][idx] == 1).all() and (p["has_lm1"][idx] != 0).all()


def test_no_scale_is_reached_where_the_class_says(problems):
    for name, want in LP.EXPECT.items():
        p = problems[name]
        if p["scale_12_in"] is not None:
            continue
        for c, st in enumerate(want):
            assert (LP.scale_restatement(p, c)[0] is None) == (st == LP.NO_SCALE or (st == -1 and LP.planted_kept(p, c) == 0)), (name, c)
    # without priors there is no ratio: the class runs on scale_12_in
    p = problems["no_priors"]
    assert p["scale_12_in"] is not None and all(LP.scale_restatement(p, c)[0] is None for c in range(p["num_candidates"]))
    # erased and swung priors give none, unindexed ones do
    assert LP.planted_kept(problems["prior_erased"], 1) == 0 and (problems["prior_erased"]["prior_state"][1] == 2).sum() == 60
    q = problems["prior_unindexed"]
    assert ((q["prior_state"][1] == 1) & (q["has_lm1"] != 0)).sum() == 70 and len(LP.scale_restatement(q, 1)[1]) == 60
    assert ((q["prior_state"][0] == 1) & (q["prior_idx2"][0] < 0)).sum() == 60


def test_shapes_are_what_the_gpu_test_relies_on(problems):
    n2 = np.diff(problems["unequal"]["kf2_off"]).tolist()
    assert n2 == [0, 1, 150, 400]
    m = problems["many_tiny"]
    assert m["num_candidates"] == 40 and np.diff(m["kf2_off"]).max() <= 30
    assert problems["each_status"]["active"].tolist() == [1, 1, 1, 0]
    assert {c["model"] for c in problems["mixed_models"]["cam2"]} == {0, 1, 2} and problems["mixed_models"]["cam1"]["model"] == 0
    t = problems["twins"]
    assert all(np.array_equal(t[k][0], t[k][1]) for k in LP.PER_CAND)
    for name, p in problems.items():
        assert (p["prior_idx2"] < np.diff(p["kf2_off"])[:, None]).all(), name
        q = p["sim3_12"][:, :4]
        assert np.abs((q * q).sum(1) - 1.0).max() < 1e-12, name


def test_scale_classes_count_tie_and_cross_the_workgroup(scale_problems):
    for name, want in LP.SCALE_KEPT.items():
        s, kept, _ = LP.scale_restatement(scale_problems[name], 0)
        assert len(kept) == want, name
        assert s == np.sort(kept)[(want - 1) // 2]
    assert scale_problems["kept_1025"]["n1"] == 1100
    _, kept, _ = LP.scale_restatement(scale_problems["ties"], 0)
    vals, counts = np.unique(kept, return_counts=True)
    assert counts.max() == 6  # six pairs share one ratio, and the median is among them or beside them
    # kept_2: the lower of the two ((2 - 1) / 2 = 0)
    s, kept, _ = LP.scale_restatement(scale_problems["kept_2"], 0)
    assert s == kept.min()


def test_boundary_pairs_sit_on_the_threshold_and_one_float_above(scale_problems):
    p = scale_problems["boundary"]
    at, above = p["boundary_idx"]
    cos = lambda i: LP.cos_and_ratio(p["pose_1w_in_cand"][0], p["pose_1w"], p["prior_pos_w"][0, i], p["pos_w1"][i])[0][0]
    assert cos(at) == LP.COS_THR and cos(above) == np.nextafter(LP.COS_THR, np.float32(2.0))
    _, kept, idx = LP.scale_restatement(p, 0)
    assert at not in idx and above in idx  # strict: the pair on the threshold is rejected
    assert ((p["prior_state"][0] == 1) & (p["has_lm1"] != 0)).sum() == 5 and len(kept) == 4


def test_header_declares_the_entry_point_and_the_binding_reads_it():
    from stella_vslam_amd import _lib
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    assert re.search(r"^int\s+svgpu_loop_sim3_batch\s*\(", hdr, flags=re.M)
    restype, argtypes = _lib.parse_header(hdr)["svgpu_loop_sim3_batch"]
    assert len(argtypes) == 58
