"""host/test_bow_compute: data::bow_vocabulary_hip::compute_bow_batch and both data::hip::bow_database::add_keyframes overloads over the
stand-in data:: classes, against the loop of compute_bow plus add_keyframe on the same descriptors, in both forms -- the maps entry for
entry with the weights as raw bit patterns, and every later acquire_keyframes.  The program is built by host/Makefile."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = ROOT / "stella_vslam_amd" / "host" / "test_bow_compute"


@pytest.mark.gpu
def test_batch_classes_equal_the_loop_over_the_per_call_classes():
    assert EXE.exists(), "build() makes stella_vslam_amd/host/test_bow_compute"
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bow compute drop-in ok" in r.stdout, r.stdout + r.stderr
