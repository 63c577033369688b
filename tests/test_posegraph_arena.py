"""The scratch layouts of the pose-graph entry points (stella_vslam_amd/csrc/posegraph_layout.h) are plain C++:
tests/posegraph_arena_check.cpp is built with g++ against that header and sv_arena.h alone and checks, for the smallest and the largest
shape of tests/test_gpu_posegraph.py, that the size the entry point measures covers every piece the same layout hands out."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_posegraph_arena_measure_covers_what_the_layout_takes(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/posegraph_arena_check.cpp")
    exe = tmp_path / "posegraph_arena_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "stella_vslam_amd" / "csrc"),
                           str(ROOT / "tests" / "posegraph_arena_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "posegraph arena ok" in r.stdout
    assert "FAIL" not in r.stdout
