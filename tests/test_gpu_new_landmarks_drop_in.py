"""host/test_new_landmarks: module::hip::new_landmark_creator::create over the stand-in data:: classes, on the toy map of test_drop_in.cpp,
against the loop mapping_module.cc:286-340 written over match::hip::robust / bow_tree::match_for_triangulation and
module::hip::two_view_triangulator with the landmarks attached between the neighbours -- the same pairs, the same positions bit for bit,
the same neighbour for every created landmark, with and without BoW nodes, with inactive neighbours, through the one batch call and
through the class's chain of single calls.  The program is built by host/Makefile."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = ROOT / "stella_vslam_amd" / "host" / "test_new_landmarks"


@pytest.mark.gpu
def test_create_equals_the_reference_loop_over_the_per_call_classes():
    assert EXE.exists(), "build() makes stella_vslam_amd/host/test_new_landmarks"
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "new landmarks drop-in ok" in r.stdout, r.stdout + r.stderr
