"""host/test_loop_sim3: module::hip::loop_sim3_validator::validate_batch over the stand-in data:: classes, on a toy map, against the stretch
module/loop_detector.cc:537-587 written per candidate with match::hip::projection::match_keyframes_mutually and
optimize::hip::transform_optimizer::optimize -- the same verdicts, the same scale and Sim3 bit for bit, the same inlier counts, the same
landmark pointers in curr_match_lms_observed_in_cand, and the first accepted candidate chosen.  The program is built by host/Makefile."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = ROOT / "stella_vslam_amd" / "host" / "test_loop_sim3"


@pytest.mark.gpu
def test_validate_batch_drop_in_equals_the_per_candidate_chain():
    assert EXE.exists(), "build() makes stella_vslam_amd/host/test_loop_sim3"
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loop sim3 drop-in ok" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("thr 20 candidate") == 3 and r.stdout.count("thr 100000 candidate") == 3, r.stdout
