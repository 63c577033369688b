"""The yardstick of the pairwise Sim3 optimizer (tests/sim3opt_problems.py) checked against itself, on the CPU.

The GPU tests demand that the device takes exactly the decisions of the long double restatement: trial sequence, statuses, inlier count,
early return.  That is a fair demand only where no decision hangs on rounding, so every planted case has to pass a filter in BOTH forms
of the restatement: every chi2 a gate reads is at least 1e-3 (relative) away from chi_sq, every gain ratio rho at least 1e-6 away from 0.
The filter is an assertion: the seeds are fixed in the module, nothing is skipped or re-drawn here."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from tests import sim3opt_problems as T

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("case", T.CASES)
def test_the_two_forms_take_identical_decisions(case):
    a, b = T.solved(case, "fp64"), T.solved(case, "ld")
    assert a["seq"] == b["seq"]
    assert np.array_equal(a["status"], b["status"])
    assert (a["num_inliers"], a["early_return"], a["lm_iterations"], a["lm_trials"]) == (b["num_inliers"], b["early_return"], b["lm_iterations"], b["lm_trials"])
    dev = T.two_form_deviation(case)
    print(f"{case}: two-form deviation {dev:.2e}, iterations {a['lm_iterations']}, trials {a['lm_trials']}, inliers {a['num_inliers']}")
    assert dev <= 1e-3


@pytest.mark.parametrize("case", T.CASES)
def test_no_decision_hangs_on_rounding(case):
    chi_sq = T.problem(case)["chi_sq"]
    for form in ("fp64", "ld"):
        gate, rho = T.filter_margins(T.solved(case, form), chi_sq)
        print(f"{case} {form}: gate margin {gate:.2e}, smallest |rho| {rho:.2e}")
        assert gate >= 1e-3
        assert rho >= 1e-6


def test_the_cases_are_what_they_claim_to_be():
    for fs in (0, 1):
        r12, r13 = T.solved(f"f12-fs{fs}", "ld"), T.solved(f"f13-fs{fs}", "ld")
        assert (r12["survivors"], r12["early_return"], r12["num_inliers"]) == (9, 1, 0)
        assert np.array_equal(np.asarray(r12["sim3"], np.float64).view(np.uint64), T.problem(f"f12-fs{fs}")["sim3"].view(np.uint64))
        assert (r13["survivors"], r13["early_return"]) == (10, 0) and r13["lm_iterations"][1] == T.NUM_ITER
        rb = T.solved(f"b-fs{fs}", "ld")
        assert int((rb["status"] == 1).sum()) >= 5  # stage 1 rejects the gross mismatches
        rc, pc = T.solved(f"c-fs{fs}", "ld"), T.problem(f"c-fs{fs}")
        assert int(((rc["status"] == 0) & (pc["p1c_z"] < 0)).sum()) >= 5  # inliers behind keyframe 1's image plane
        assert pc["cam1"]["model"] == pc["cam2"]["model"] == T.EQUIRECTANGULAR and (pc["cam1"]["cols"], pc["cam1"]["rows"]) == (1920.0, 960.0)
        pd = T.problem(f"d-fs{fs}")
        assert pd["cam1"]["model"] != T.EQUIRECTANGULAR and pd["cam2"]["model"] == T.EQUIRECTANGULAR and len(set(pd["w1"].tolist())) > 1
    assert abs(T.problem("e0.5-fs0")["true"][7] - 0.5) < 1e-12 and abs(T.problem("e2-fs0")["true"][7] - 2.0) < 1e-12
    sizes = sorted(len(T.problem(c)["obs1"]) for c in T.CASES if c.startswith("g"))
    assert sizes == sorted(T.SIZES) and {T.WORKGROUP_EDGES // 2 - 1, T.WORKGROUP_EDGES // 2, T.WORKGROUP_EDGES // 2 + 1, 31, 32, 33} <= set(sizes)
    # under fix_scale the restatement keeps the scale bit for bit
    for case in T.CASES:
        if case.endswith("fs1"):
            assert float(T.solved(case, "fp64")["sim3"][7]) == float(T.problem(case)["sim3"][7])


def test_num_iter_zero_reads_the_first_stage_cache():
    p = T.problem("b-fs0")
    r = T.optimize(p, np.longdouble, num_iter=0)
    assert r["lm_iterations"] == [5, 0] and r["early_return"] == 0
    assert r["num_inliers"] == r["survivors"] == int((r["status"] == 0).sum()) and not (r["status"] == 2).any()


def test_header_declares_and_library_exports_the_entry_points():
    text = (ROOT / "include" / "svgpu.h").read_text()
    for name in ("svgpu_sim3_transform_optimize_batch", "svgpu_sim3_transform_optimize"):
        assert re.search(r"\bint " + name + r"\(svgpu_ctx\* ctx,", text), name
    assert "#define SVGPU_ABI_VERSION 1" in text
    lib = C.CDLL(str(ROOT / "stella_vslam_amd" / "libsvgpu.so"))
    for name in ("svgpu_sim3_transform_optimize_batch", "svgpu_sim3_transform_optimize"):
        assert hasattr(lib, name), name
