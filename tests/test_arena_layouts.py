"""The scratch arena (stella_vslam_amd/csrc/sv_arena.h) and the layouts of the entry points whose pieces carry their counts (pnp_layout.h,
posegraph_layout.h, posegraph_envelope_layout.h, sim3opt_layout.h, poseopt_batch_layout.h, match_layout.h, ba_layout.h, track_layout.h,
frame_layout.h) are plain C++.  Each check program is built with
g++ against those headers alone.  arena_check.cpp checks the arena itself, the read-back range merge and the shared argument checks; the
other eight run tests/layout_check.h for the smallest and the largest shape of their GPU test: measuring hands out no pointer and keeps
every count, the measured size covers every piece the same layout places, the bytes per piece written out by hand in the program are the
pieces' own, no two pieces overlap, and a capacity one byte short latches the overflow flag.  match_arena_check.cpp adds the prefix invariant
of the two-pass matchers: every piece in front of the candidate lists keeps its offset whatever the lists' capacity.  ba_arena_check.cpp
checks both placements of bundle adjustment (device arena and page-locked host image, under every flag combination), that their input
blocks coincide piece by piece, that the output block is what the one-copy read-back takes it for, and ba_block_rows against a
brute-force restatement.  track_arena_check.cpp checks the persistent buffers of the tracked-frame chain (track_layout.h) and the resident
frame's slab (frame_layout.h, built with include/svgpu.h and orb_plan.h beside it): the input block's two id lists inside one piece (the
second at a 256-byte boundary behind the keypoint capacity, both within the piece, the image adjacent in front), the observation's layout
over a buffer of its own against the head of the slab, offset for offset and byte for byte with the expressions the tracker used to write
out, and the growth policy track_caps (floors, never shrinking, idempotent, no re-allocation for a call repeated).  ba_plan_check.cpp checks
the decisions of bundle adjustment (ba_plan.h, no arena in it): the environment switches parsed from a table, every plan function against
the expression it replaced at the thresholds' neighbours and the bench shapes, and the key of the envelope plan cache.  ba_stage_check.cpp
(built with -pthread) checks the observation staging of bundle adjustment (ba_stage.h, the only code of the library that starts threads):
teams of 1, 2, 3, 5, 8 and 16 threads against a single-thread restatement on shapes that put every boundary of the shares to work --
landmark offsets, the staged image byte for byte, the poses seen, the stable order of ungrouped observations, an index out of range in
every share -- and, through a recording uploader over a fake device arena, that a released team uploads every element once, whole arrays
or chunk by chunk, that an abandoned one uploads nothing, and that either way it joins with points_out holding the input points."""
import pytest

from tests.host_check import ROOT, build_and_run

PROGRAMS = {
    "arena_check.cpp": "arena ok",
    "pnp_arena_check.cpp": "pnp arena ok",
    "posegraph_arena_check.cpp": "posegraph arena ok",
    "posegraph_envelope_arena_check.cpp": "posegraph envelope arena ok",
    "sim3opt_arena_check.cpp": "sim3opt arena ok",
    "poseopt_batch_arena_check.cpp": "poseopt batch arena ok",
    "match_arena_check.cpp": "match arena ok",
    "ba_arena_check.cpp": "ba arena ok",
    "track_arena_check.cpp": "track arena ok",
    "ba_plan_check.cpp": "ba plan ok",
    "ba_stage_check.cpp": "ba stage ok",
}
EXTRA_FLAGS = {"ba_stage_check.cpp": ("-pthread",)}  # the one program that starts threads


@pytest.mark.parametrize("source", list(PROGRAMS))
def test_measure_covers_what_the_layout_takes(source, tmp_path):
    build_and_run(source, PROGRAMS[source], tmp_path, EXTRA_FLAGS.get(source, ()))


def test_the_checked_shapes_are_those_of_the_gpu_test():
    from tests import poseopt_batch_problems as PB
    src = (ROOT / "tests" / "poseopt_batch_arena_check.cpp").read_text()
    for call, ps in PB.classes().items():
        assert f"check({len(ps)}, {sum(len(p['pos_w']) for p in ps)});" in src, call
    assert "check(300, 19500);" in src and "check(1, 0);" in src
