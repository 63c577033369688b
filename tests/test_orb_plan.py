"""The host planner of the ORB front end (stella_vslam_amd/csrc/orb_plan.h) is plain C++: tests/orb_plan_check.cpp is built with g++ against
that header alone and checks, for the shapes of tests/test_gpu_orb.py and the edge shapes (a level too wide for the LDS-resident pyramid,
levels without cells, a refused geometry), that the tables it returns keep what the kernels rely on: describe bands, pyramid bands, FAST
cells and selection grid, resize tables, blur work items, and the per-call launch decisions at both sides of their thresholds."""
from tests.host_check import build_and_run


def test_orb_plan_keeps_what_the_kernels_rely_on(tmp_path):
    # -ffp-contract=off: the planner's fp32 / fp64 expressions are the reference's, unfused (the library is built with the same flag)
    build_and_run("orb_plan_check.cpp", "orb plan ok", tmp_path, extra_flags=["-ffp-contract=off"])
