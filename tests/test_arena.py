"""The scratch arena (stella_vslam_amd/csrc/sv_arena.h) is plain C++: tests/arena_check.cpp is built with g++ against that header alone
and checks that measuring and placing agree, that measuring hands out no pointer, and that a capacity one byte short latches the overflow
flag instead of returning an out-of-range pointer."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_arena_measure_equals_place(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/arena_check.cpp")
    exe = tmp_path / "arena_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "stella_vslam_amd" / "csrc"),
                           str(ROOT / "tests" / "arena_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "arena ok" in r.stdout
    assert "FAIL" not in r.stdout
