"""The host planner of the ORB front end (stella_vslam_amd/csrc/orb_plan.h) is plain C++: tests/orb_plan_check.cpp is built with g++ against
that header alone and checks, for the shapes of tests/test_gpu_orb.py and the edge shapes (a level too wide for the LDS-resident pyramid,
levels without cells, a refused geometry), that the tables it returns keep what the kernels rely on: describe bands, pyramid bands, FAST
cells and selection grid, resize tables, blur work items, and the per-call launch decisions at both sides of their thresholds."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_orb_plan_keeps_what_the_kernels_rely_on(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/orb_plan_check.cpp")
    exe = tmp_path / "orb_plan_check"
    # -ffp-contract=off: the planner's fp32 / fp64 expressions are the reference's, unfused (the library is built with the same flag)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", str(ROOT / "stella_vslam_amd" / "csrc"),
                           str(ROOT / "tests" / "orb_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orb plan ok" in r.stdout
    assert "FAIL" not in r.stdout
