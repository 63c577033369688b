"""The host-only check programs (tests/*_check.cpp) are plain C++ with a main of their own: each is built with g++ against the headers of
stella_vslam_amd/csrc it names (and include/svgpu.h, for the layouts that hold its records), run, and passes when it exits with 0 and prints its marker."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]


def build_and_run(source, marker, tmp_path, extra_flags=()):
    """Build tests/<source> into tmp_path and run it; the program's output."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail(f"g++ is needed to build tests/{source}")
    exe = tmp_path / pathlib.Path(source).stem
    subprocess.check_call([cxx, *FLAGS, *extra_flags, "-I", str(ROOT / "stella_vslam_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / source), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert marker in r.stdout
    assert "FAIL" not in r.stdout
    return r.stdout
