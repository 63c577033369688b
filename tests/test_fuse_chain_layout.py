"""The scratch layout of svgpu_fuse_landmarks_batch (stella_vslam_amd/csrc/fuse_layout.h) under the harness of tests/layout_check.h: the
counted pieces, the results as one range, the prefix invariant across the two passes and the two sizing rules -- also as a stand-alone host
program under AddressSanitizer and UBSan."""
from tests import host_check


def test_fuse_arena_layout(tmp_path):
    out = host_check.build_and_run("fuse_arena_check.cpp", "fuse arena ok", tmp_path)
    assert out.count("ok ") == 9, out


def test_fuse_arena_layout_under_sanitizers(tmp_path):
    out = host_check.build_and_run("fuse_arena_check.cpp", "fuse arena ok", tmp_path, extra_flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert out.count("ok ") == 9, out
