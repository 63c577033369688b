"""The scratch layout of svgpu_sim3_transform_optimize_batch (stella_vslam_amd/csrc/sim3opt_layout.h) is plain C++:
tests/sim3opt_arena_check.cpp is built with g++ against that header and sv_arena.h alone and checks, for the smallest and the largest
shape of tests/test_gpu_sim3opt.py, that the size the entry point measures covers every piece the same layout hands out."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_sim3opt_arena_measure_covers_what_the_layout_takes(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/sim3opt_arena_check.cpp")
    exe = tmp_path / "sim3opt_arena_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "stella_vslam_amd" / "csrc"),
                           str(ROOT / "tests" / "sim3opt_arena_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sim3opt arena ok" in r.stdout
    assert "FAIL" not in r.stdout
