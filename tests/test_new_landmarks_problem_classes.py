"""The problems of tests/new_landmarks_problems.py are what they claim, by the CPU restatement of the loop alone: the classes built around
the carry of the landmark state give different matches AND different accepted sets when the carry is dropped (the composition of the two
independent batch calls), so a device chain that forgets it cannot pass the GPU test; the rejected groups reach the four statuses they are
planted for and stay queries; the sizes are the ones the device paths branch on; the C header carries the entry point.  No GPU."""
import pathlib
import re

import numpy as np
import pytest

from tests import new_landmarks_problems as NP
from tests import triangulation_problems as T

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", ["order_effect", "rejected_stay", "all_taken_after_first"])
def test_carry_changes_matches_and_accepted_sets(name):
    p = NP.problem(name)
    a, b = NP.chain(p), NP.chain(p, carry=False)
    assert np.array_equal(a["matched_2_in_1"][0], b["matched_2_in_1"][0])          # neighbour 0 sees taken_0 either way
    later = slice(1, None)
    assert (a["matched_2_in_1"][later] != b["matched_2_in_1"][later]).any()
    assert ((a["status"][later] == T.ACCEPTED) != (b["status"][later] == T.ACCEPTED)).any()
    # with the carry a keypoint gets at most one landmark; without it some get two
    assert ((a["status"] == T.ACCEPTED).sum(0) <= 1).all() and ((b["status"] == T.ACCEPTED).sum(0) > 1).any()
    assert np.array_equal(a["created_by"] >= 0, (a["status"] == T.ACCEPTED).any(0))


def test_order_effect_hands_the_claimed_keypoint_to_a_later_query():
    """(a): a planted keypoint accepted at neighbour 0 would, without the carry, claim its twin in neighbour 1 again; with it the twin goes to the
    shadow keypoint behind it in index order."""
    p = NP.problem("order_effect")
    a, b = NP.chain(p), NP.chain(p, carry=False)
    moved = 0
    for sh in p["shadows"]:
        t = a["matched_2_in_1"][1][sh]
        if t < 0 or b["matched_2_in_1"][1][sh] == t:
            continue
        owner = np.flatnonzero(b["matched_2_in_1"][1] == t)   # who holds that side-2 keypoint without the carry
        assert len(owner) == 1 and owner[0] < sh and a["status"][0][owner[0]] == T.ACCEPTED and a["matched_2_in_1"][1][owner[0]] == -1
        moved += 1
    assert moved >= 3, moved


def test_rejected_keypoints_reach_their_status_and_stay_queries():
    """(b): matched at neighbour 0, rejected there by the status the group is planted for, matched again at neighbour 1."""
    p = NP.problem("rejected_stay")
    a = NP.chain(p)
    kp = p["kp_of_pt"][0]
    for key, want in (("no_mode", T.NO_MODE), ("depth", T.DEPTH), ("reproj", T.REPROJECTION), ("scale", T.SCALE)):
        idx = kp[p["groups"][key]]
        hit = idx[a["status"][0][idx] == want]
        assert len(hit) >= 2, (key, a["status"][0][idx])
        assert (a["matched_2_in_1"][0][hit] >= 0).all() and (a["matched_2_in_1"][1][hit] >= 0).any(), key
        assert (a["created_by"][hit] != 0).all()


def test_all_taken_after_first_leaves_later_problems_empty():
    p = NP.problem("all_taken_after_first")
    a = NP.chain(p)
    assert a["num_accepted"][0] > 50 and (a["num_matches"][1:] == 0).all() and a["taken"].all()
    assert (NP.chain(p, carry=False)["num_matches"][1:] > 0).all()


def test_inactive_and_empty_shapes():
    p = NP.problem("inactive_middle")
    a = NP.chain(p)
    assert list(p["active"]) == [1, 0, 1] and a["num_matches"][1] == 0 and (a["status"][1] == T.SKIPPED).all() and a["num_accepted"][[0, 2]].min() > 0
    q = NP.problem("all_inactive")
    assert not q["active"].any() and NP.chain(q)["num_matches"].sum() == 0
    e = NP.problem("empty_neighbour")
    assert [len(s["desc"]) > 0 for s in e["side2"]] == [True, False, True] and NP.chain(e)["num_accepted"][[0, 2]].min() > 0
    assert len(NP.problem("empty_current")["side1"]["desc"]) == 0 and len(NP.problem("single")["side2"]) == 1
    assert NP.problem("robust")["side1"]["node"] is None and NP.problem("order_effect")["side1"]["node"] is not None


def test_stereo_models_buckets_and_spill_reach_their_paths():
    s = NP.problem("stereo")
    a = NP.chain(s)
    acc = a["status"] == T.ACCEPTED
    assert (acc & (a["branch"] == T.STEREO_1)).any() and (acc & (a["branch"] == T.STEREO_2)).any() and (acc & (a["branch"] == T.LINEAR)).any()
    m = NP.problem("models")
    assert [v["cam"]["model"] for v in m["neighbours"]] == [T.FISHEYE, T.EQUIRECTANGULAR, T.RADIAL_DIVISION]
    assert (NP.chain(m)["num_accepted"] > 0).all()
    b = NP.problem("buckets_64_65")
    assert [(x["node"] == 0).sum() for x in b["side2"]] == [64, 65] and 0 < b["side1"]["has_lm"].mean() < 1
    sp = NP.problem("spill")
    n1, n2 = len(sp["side1"]["desc"]), [len(x["desc"]) for x in sp["side2"]]
    assert NP.cand_lds_bytes(n1, n2[1]) > NP.CAND_LDS_BUDGET and max(NP.cand_lds_bytes(n1, n2[0]), NP.cand_lds_bytes(n1, n2[2])) < NP.CAND_LDS_BUDGET
    assert (NP.chain(sp)["num_accepted"] > 0).all()


@pytest.mark.parametrize("name", NP.CLASSES)
def test_shapes_and_decision_margins(name):
    """64 to 300 keypoints a side (the spill's large neighbour and the empty sides apart), K of 1 to 5, and no matched pair within rounding
    distance of a triangulator threshold: the device may be held to the restatement's statuses exactly."""
    p = NP.problem(name)
    assert 1 <= len(p["side2"]) <= 5
    for s in [p["side1"]] + list(p["side2"]):
        n = len(s["desc"])
        assert n == 0 or 64 <= n <= 300 or (name == "spill" and n == NP.SPILL_N2), (name, n)
    a = NP.chain(p)
    live = a["status"] != T.SKIPPED
    assert (a["margin"][live] > 1e-9).all()


def test_header_declares_the_entry_point():
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    assert re.search(r"^int\s+svgpu_new_landmarks_batch\s*\(", hdr, flags=re.M)
    assert "#define SVGPU_ABI_VERSION 1" in hdr
