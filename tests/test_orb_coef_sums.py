"""The resize coefficient tables of the ORB planner (stella_vslam_amd/csrc/orb_plan.h) keep a0 + a1 <= 2049 and b0 + b1 <= 2049: the
pack of k_pyramid_lds stores its results without masking them to a byte and relies on it.  tests/orb_coef_sum_check.cpp is built with g++
against the header alone: the property on the shapes of tests/test_orb_plan.py, a table broken on purpose (a pair summing to 2050) is
refused, and the worst case of the vertical blend fits a byte."""
from tests.host_check import build_and_run


def test_resize_coefficient_sums_are_verified(tmp_path):
    build_and_run("orb_coef_sum_check.cpp", "orb coefficient sums ok", tmp_path, extra_flags=["-ffp-contract=off"])
