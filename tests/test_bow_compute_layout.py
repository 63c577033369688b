"""The scratch layout of svgpu_bow_compute_batch (stella_vslam_amd/csrc/bow_compute_layout.h) under the harness of tests/layout_check.h:
counted pieces, no overlap, the upload and the results as one range each, the cap of the workgroup path and the switch to the general sort."""
from tests import host_check


def test_bow_compute_arena_layout(tmp_path):
    out = host_check.build_and_run("bow_compute_arena_check.cpp", "bow compute arena ok", tmp_path)
    assert out.count("ok ") == 6, out
