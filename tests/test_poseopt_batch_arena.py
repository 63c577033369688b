"""The scratch layout of svgpu_pose_optimize_batch (stella_vslam_amd/csrc/poseopt_batch_layout.h) is plain C++:
tests/poseopt_batch_arena_check.cpp is built with g++ against that header and sv_arena.h alone and checks, for the smallest and the largest
batch of tests/test_gpu_poseopt_batch.py, that the size the entry point measures covers every piece the same layout hands out."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_poseopt_batch_arena_measure_covers_what_the_layout_takes(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/poseopt_batch_arena_check.cpp")
    exe = tmp_path / "poseopt_batch_arena_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "stella_vslam_amd" / "csrc"),
                           str(ROOT / "tests" / "poseopt_batch_arena_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poseopt batch arena ok" in r.stdout
    assert "FAIL" not in r.stdout


def test_the_checked_shapes_are_those_of_the_gpu_test():
    from tests import poseopt_batch_problems as PB
    src = (ROOT / "tests" / "poseopt_batch_arena_check.cpp").read_text()
    for call, ps in PB.classes().items():
        assert f"check({len(ps)}, {sum(len(p['pos_w']) for p in ps)});" in src, call
    assert "check(300, 19500);" in src and "check(1, 0);" in src
