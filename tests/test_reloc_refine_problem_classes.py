"""The classes of tests/reloc_refine_problems.py reach the branches they are named for -- shown on the CPU, with the oracle's restatements of
the projection matcher and the pose optimiser standing behind `compose_single_calls`.  The deciding counts of every class that is not a
planted boundary lie at least 5 away from min_num_valid_obs, so a last-bit difference between oracle and device cannot move a class.
The 260 tiny candidates of `many_tiny` are left out here (a load class, 260 copies of one kind of candidate with its own threshold of 20; the
GPU test compares it with the yardstick like the others).  Also here: the layout of the call's scratch arena (host check), and the header / binding agreement on the new entry point."""
import pathlib
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import host_check
from tests import reloc_refine_problems as RP

ROOT = pathlib.Path(__file__).resolve().parent.parent


def oracle_backend(problem):
    c = problem["cam"]
    cam = O.make_camera(c["model"], c["cols"], c["rows"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"], c["focal_x_baseline"])

    def do_match(problem, check, **kw):
        return O.match_frame_and_keyframe_projection(bool(check), cam, **kw)[0]

    def do_opt(problem, pose, pos_w, uvr, w, hb):
        nv, out, flags, st = O.pose_optimize(pose, pos_w, uvr, w, hb, problem["intrinsics"], problem["num_trials_robust"], problem["num_trials"],
                                             problem["num_each_iter"], reset_flag_each_round=bool(problem["reset_stop_flag_each_round"]))
        return nv, out, flags, 0
    return do_match, do_opt


@pytest.fixture(scope="module")
def results():
    P = RP.classes()
    return P, {name: RP.compose_single_calls(p, oracle_backend(p)) for name, p in P.items() if name != "many_tiny"}


def test_every_class_reaches_its_status(results):
    P, R = results
    for name, r in R.items():
        assert r["status"].tolist() == RP.EXPECT[name], (name, r["status"], r["num_found"], r["num_valid"])
    seen = {s for r in R.values() for s in r["status"].tolist()}
    assert {-1, 0, 1, 2, 3} <= seen  # accepted, inactive, every status value of one and two stages; four stages: the count tests of stages 0 and 2


def test_deciding_counts_lie_five_away_from_the_threshold(results):
    P, R = results
    for name, r in R.items():
        p = P[name]
        S, m = p["num_stages"], p["min_num_valid_obs"]
        for c in range(p["num_candidates"]):
            st = int(r["status"][c])
            if st < 0:
                continue
            count = int(p["n_already_found"][c])
            for s in range(S):
                dec = count + int(r["num_found"][c, s])
                if st == 1 + s:
                    assert dec <= m - 5, (name, c, s, dec)
                    break
                assert dec >= m + 5, (name, c, s, dec)
                count = int(r["num_valid"][c, s])
            else:
                assert (count <= m - 5) if st == 1 + S else (count >= m + 5), (name, c, count)


def test_stages_that_match_and_the_skip(results):
    P, R = results
    # the rolled input pose leaves keypoints for the later stages; the small perturbation does not need them
    late = R["all_accepted"]
    assert late["num_found"][2, 1] >= 3 and late["num_found"][2, 0] >= 50
    assert (late["match_stage"][RP.rows_of(P["all_accepted"], [2])] == 1).sum() == late["num_found"][2, 1]
    four = R["four_stages"]
    assert (four["num_found"][1] > 0).sum() >= 2
    # fewer than five observations: the optimiser is skipped, the pose is the input bit for bit, no flag
    d, dp = R["degenerate"], P["degenerate"]
    assert d["num_valid"][2, 0] == 0 and not d["outlier"][2].any() and d["pose_out"][2].tobytes() == dp["pose_cw"][2].tobytes()
    assert dp["frame_has_lm"][2].sum() + d["num_found"][2, 0] < 5
    # no entry offered / empty slice: nothing found, accepted on what the frame holds; empty frame: everything from the matcher
    assert d["num_found"][0].sum() == 0 and d["num_found"][3].sum() == 0 and dp["kf_off"][3] == dp["kf_off"][4]
    assert dp["frame_has_lm"][1].sum() == 0 and dp["n_already_found"][1] == 0 and d["num_found"][1, 0] >= 55
    # wrong positions are outliers of the optimisation: that is what fails the final test
    e = R["each_status"]
    assert e["num_found"][4, 0] == 0 and e["num_found"][4, 1] >= 20 and e["outlier"][4].sum() >= 10
    # stereo edges on part of the keypoints only
    xr = P["stereo"]["t_xright"]
    assert 0 < (xr >= 0).sum() < len(xr)
    # twins: identical keyframe data, different poses, different results
    t, tp = R["twins"], P["twins"]
    a, b = RP.rows_of(tp, [0]), RP.rows_of(tp, [1])
    assert np.array_equal(tp["pos_w"][a], tp["pos_w"][b]) and tp["pose_cw"][0].tobytes() != tp["pose_cw"][1].tobytes()
    assert t["pose_out"][0].tobytes() != t["pose_out"][1].tobytes()


def test_scene_sizes():
    P = RP.classes()
    for name, p in P.items():
        n = np.diff(p["kf_off"])
        if name == "many_tiny":
            assert p["num_candidates"] == 260 and p["nt"] == 64 and (n == 40).all()
            continue
        assert 200 <= p["nt"] <= 400 and 1 <= p["num_candidates"] <= 8
        assert all(k == 0 or 150 <= k <= 400 for k in n), (name, n)
    assert {p["num_stages"] for p in P.values()} == {1, 2, 4}


def test_sub_problem_keeps_rows():
    p = RP.classes()["each_status"]
    q = RP.sub(p, [3, 1])
    assert q["num_candidates"] == 2 and np.array_equal(q["pos_w"], p["pos_w"][RP.rows_of(p, [3, 1])])
    assert np.array_equal(q["pose_cw"][0], p["pose_cw"][3])


def test_reloc_refine_arena_layout(tmp_path):
    out = host_check.build_and_run("reloc_refine_arena_check.cpp", "reloc refine arena ok", tmp_path)
    assert out.count("ok K ") == 5, out


def test_header_declares_the_entry_point_and_the_binding_reads_it():
    from stella_vslam_amd import _lib
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    assert re.search(r"^int\s+svgpu_reloc_refine_batch\s*\(", hdr, flags=re.M)
    restype, argtypes = _lib.parse_header(hdr)["svgpu_reloc_refine_batch"]
    assert len(argtypes) == 46
