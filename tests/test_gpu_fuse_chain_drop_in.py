"""host/test_landmark_fuser: module::hip::landmark_fuser::fuse over the stand-in data:: classes on a toy map with six fuse targets, planted
duplicates and new connections -- through the one batch call, through the class's own chain of single match::hip::fuse calls, on the
overflow fall-back, and against mapping_module.cc:417-537 written out over match::hip::fuse and the stand-in landmark methods.  All agree on
every landmark's observation map, the will_be_erased set, replaced_lms and every keyframe's landmark vector; descriptors bit for bit;
normals and distance limits within the tolerances of test_mapping_keyframe_batched_refresh_equals_the_per_landmark_methods.  The program is
built by host/Makefile."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = ROOT / "stella_vslam_amd" / "host" / "test_landmark_fuser"


@pytest.mark.gpu
def test_fuse_equals_the_reference_loop_over_the_per_call_classes():
    assert EXE.exists(), "build() makes stella_vslam_amd/host/test_landmark_fuser"
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "landmark fuser drop-in ok" in r.stdout, r.stdout + r.stderr
