"""The scratch layout of svgpu_loop_sim3_batch (stella_vslam_amd/csrc/loop_sim3_layout.h) under the harness of tests/layout_check.h, for the
smallest and the largest shape of tests/test_gpu_loop_sim3.py; and that the two record sizes of the check program that plain C++ can
measure (the optimiser's problem descriptor and its stats) are the library's own."""
import pathlib
import re

from tests import host_check

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_loop_sim3_arena_layout(tmp_path):
    out = host_check.build_and_run("loop_sim3_arena_check.cpp", "loop sim3 arena ok", tmp_path)
    assert out.count("ok K ") == 6, out


def test_problem_and_stats_record_sizes_of_the_check_are_the_librarys(tmp_path):
    """PROB and STATS of the check program against the library's own plain-C++ headers.  REPROJ, CAND, REPLAY and GRID are sizes of HIP-side
    structs: they only scale pieces of the layout, the call itself passes sizeof, and here REPROJ is merely bounded below by the camera."""
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include "sim3opt_layout.h"\n#include "svgpu.h"\n'
                   'int main() { std::printf("%d %zu %zu\\n", S3O_LAYOUT_PROBLEM, sizeof(svgpu_sim3opt_stats), sizeof(svgpu_camera)); }\n')
    import subprocess
    exe = tmp_path / "sizes"
    subprocess.check_call(["g++", "-std=c++17", "-I", str(ROOT / "stella_vslam_amd" / "csrc"), "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    prob, stats, cam = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    chk = (ROOT / "tests" / "loop_sim3_arena_check.cpp").read_text()
    m = re.search(r"PROB = (\d+), REPROJ = (\d+), CAND = (\d+), REPLAY = (\d+), GRID = (\d+), STATS = (\d+)", chk)
    assert int(m.group(1)) == prob and int(m.group(6)) == stats
    assert int(m.group(2)) >= cam  # a ReprojProblem holds the camera
