"""host/test_relocalizer_batch: module::hip::relocalizer::refine_pose_batch over the stand-in data:: classes against relocalizer::refine_pose
written with the per-call drop-in classes -- the same verdicts, the same poses bit for bit, the same landmark pointers at the same keypoints
(matched landmarks added, the last optimisation's outliers dropped for an accepted candidate).  The program is built by host/Makefile."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = ROOT / "stella_vslam_amd" / "host" / "test_relocalizer_batch"


@pytest.mark.gpu
def test_refine_pose_batch_drop_in_equals_refine_pose_per_candidate():
    assert EXE.exists(), "build() makes stella_vslam_amd/host/test_relocalizer_batch"
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "relocalizer batch ok" in r.stdout, r.stdout + r.stderr


def test_host_halves_alone_without_a_device():
    assert EXE.exists(), "build() makes stella_vslam_amd/host/test_relocalizer_batch"
    r = subprocess.run([str(EXE), "--host-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "relocalizer batch host halves ok" in r.stdout and "relocalizer batch ok" not in r.stdout, r.stdout + r.stderr
