"""The scratch layout of svgpu_new_landmarks_batch (stella_vslam_amd/csrc/newlm_layout.h) under the harness of tests/layout_check.h: the
counted pieces, the results as one range, and the prefix invariant across the two passes."""
from tests import host_check


def test_new_landmarks_arena_layout(tmp_path):
    out = host_check.build_and_run("newlm_arena_check.cpp", "new landmarks arena ok", tmp_path)
    assert out.count("ok ") == 9, out
