"""The problem classes of svgpu_fuse_landmarks_batch without a device (tests/fuse_chain_problems.py): per class the carry from target to
target changes the result against K independent detect_duplication calls on the snapshot, every class stays inside the observation-list
capacities, the one built to overflow does, and the entry point refuses NULL arguments without a device."""
import numpy as np
import pytest

from tests import fuse_chain_problems as F

CARRY = [n for n in F.ALL if n != "all_minus_one"]  # (an all -1 forward list has no forward pass to carry anything)


@pytest.fixture(scope="module")
def results():
    out = {}
    for name in F.ALL:
        p = F.prepared(name)
        out[name] = (p, F.cpu_chain(p), F.cpu_chain(p, carry=False))
    return out


@pytest.mark.parametrize("name", CARRY)
def test_the_carry_changes_the_result(results, name):
    p, carried, independent = results[name]
    assert (carried["best_idx"] != independent["best_idx"]).any()
    assert (carried["event"] != F.NONE).any()


@pytest.mark.parametrize("name", F.ALL)
def test_classes_stay_inside_both_capacity_rules(results, name):
    """no class overflows by accident: every observation list stays inside its capacity, and the lists of every pass of the chain inside the
    arena that fuse_cand_capacity sizes from the snapshot's totals"""
    p, carried, independent = results[name]
    assert (carried["obs_cnt"] <= p["table"]["obs_cap"]).all()
    assert (p["table"]["obs_cap"] <= 4096).all()
    cap = F.CAND_FACTOR * int(independent["cand_totals"].max(initial=0)) + F.CAND_SLACK
    assert carried["cand_totals"].max(initial=0) <= cap


def test_the_arena_overflow_class_outgrows_the_arena():
    p = F.prepared("arena_overflow")
    carried = F.cpu_chain(p)
    assert carried["cand_totals"][1] > F.cand_capacity(p) >= carried["cand_totals"][0]


def _first_pass_pairs(p, c):
    """the duplicate hits of the pass into target 1, whose inputs are the table on entry: (event, num_observations of the checked landmark,
    of the keypoint's landmark)"""
    t, n = p["table"], len(p["fwd_list"])
    nobs = lambda l: int(t["obs_weight"][t["obs_off"][l]:t["obs_off"][l] + t["obs_cnt"][l]].sum())  # noqa: E731
    out = []
    for i in range(n):
        ev, b = c["event"][i], c["best_idx"][i]
        if ev in (F.DUP_SURVIVED, F.DUP_LOST):
            out.append((int(ev), nobs(int(p["fwd_list"][i])), nobs(int(p["keyframes"][1]["kp_lm"][b]))))
    return out


def test_the_swap_in_both_directions_and_at_equality(results):
    """:442: the checked landmark loses only with strictly fewer num_observations()"""
    seen = set()
    for name in ("basic", "swap", "stereo", "cap_exact", "k4"):
        p, c, _ = results[name]
        for ev, na, nb in _first_pass_pairs(p, c):
            assert ev == (F.DUP_LOST if na < nb else F.DUP_SURVIVED), (name, na, nb)
            seen.add("less" if na < nb else "equal" if na == nb else "more")
    assert seen == {"less", "equal", "more"}
    assert all(na == nb for _, na, nb in _first_pass_pairs(*results["cap_exact"][:2]))  # the class of equality alone


def test_a_loser_at_target_1_would_have_matched_at_target_2(results):
    p, c, i = results["swap"]
    n = len(p["fwd_list"])
    lost = np.flatnonzero(c["event"][:n] == F.DUP_LOST)
    assert len(lost) > 0
    dead = p["fwd_list"][lost]
    assert (c["alive"][dead] == 0).all() and (c["best_idx"][n:2 * n][lost] < 0).all()   # erased: no query for target 2 ...
    assert (i["best_idx"][n:2 * n][lost] >= 0).any()                                      # ... where the snapshot lets it match


def test_backward_candidates_that_the_forward_loop_killed_or_refreshed(results):
    K = 2
    # killed: landmarks of the targets that lost a duplicate are no backward candidates, though the snapshot matches them into the current keyframe
    p, c, i = results["basic"]
    o = K * len(p["fwd_list"])
    killed = c["alive"][p["bwd_list"]] == 0
    assert killed.any() and (c["best_idx"][o:][killed] < 0).all() and (i["best_idx"][o:][killed] >= 0).any()
    # refreshed: a target's landmark that won took the current keyframe's observation, so it is observed there and no query either
    p, c, i = results["swap"]
    o = K * len(p["fwd_list"])
    t = p["table"]
    cur = p["keyframes"][0]["observer"]
    has_cur = np.array([cur in c["obs_observer"][t["obs_off"][l]:t["obs_off"][l] + c["obs_cnt"][l]] for l in p["bwd_list"]])
    won = (c["alive"][p["bwd_list"]] != 0) & has_cur
    assert won.any() and (c["best_idx"][o:][won] < 0).all() and (i["best_idx"][o:][won] >= 0).any()


def test_a_refreshed_descriptor_flips_a_later_match(results):
    p, c, i = results["desc_flip"]
    n, npts = len(p["fwd_list"]), 60
    rows = np.arange(npts)
    assert (c["event"][:n][rows] == F.NEW_CONNECTION).all()
    assert np.array_equal(c["descriptor"][:npts], p["keyframes"][1]["desc"][:npts])       # the refreshed descriptor is target 1's keypoint
    assert (i["best_idx"][n:2 * n][rows] == rows).all() and (c["best_idx"][n:2 * n][rows] < 0).all()


def test_refreshed_distance_limits_move_the_level_and_the_window(results):
    p, c, i = results["level_move"]
    n, npts = len(p["fwd_list"]), 60
    rows = np.arange(npts)
    assert (c["max_valid_dist"][:npts] > 3.0 * p["table"]["max_valid_dist"][:npts]).all()  # limits of the top level behind the connection
    assert (i["best_idx"][n:2 * n][rows] == rows).all()                                     # the snapshot: level 0, the own keypoint
    got = c["best_idx"][n:2 * n][rows]
    assert (got >= npts).all() and (p["keyframes"][2]["octave"][got] == 6).all()           # the chain: a level-6 keypoint of the wider window
    assert c["cand_totals"][1] > i["cand_totals"][1]


def test_four_camera_models(results):
    for name, model in (("basic", "perspective"), ("fisheye", "fisheye"), ("equirectangular", "equirectangular"), ("radial", "radial_division")):
        p, c, _ = results[name]
        assert p["keyframes"][1]["model"] == model and (c["num_fused"][:2] > 20).all()


def test_what_the_classes_are_built_for(results):
    ev = {n: np.bincount(results[n][1]["event"], minlength=6) for n in F.CLASSES}
    assert ev["swap"][F.DUP_LOST] > 0 and ev["swap"][F.DUP_SURVIVED] == 0      # the target's landmark outweighs the checked one (:442)
    assert ev["same_id"][F.SAME_ID] == 3
    assert ev["stereo"][F.NEW_CONNECTION] > 0 and (results["stereo"][1]["obs_weight"] == 2).any()
    assert results["empty_target"][1]["num_fused"][0] == 0
    assert results["all_minus_one"][1]["num_fused"][:2].sum() == 0 and results["all_minus_one"][1]["num_fused"][2] > 0
    p, c, _ = results["k12"]
    assert len(p["keyframes"]) == 13 and (c["num_fused"][:12] > 0).all()
    p, c, _ = results["cap_exact"]  # every list filled to exactly its capacity
    live = c["alive"] != 0
    assert (c["obs_cnt"][live] == p["table"]["obs_cap"][live]).all()
    # a replaced_by chain of length 2 in front of a new connection: the connecting row's keypoint ends up held by the chain's LAST survivor
    p, c, _ = results["chain2"]
    rb, n = c["replaced_by"], len(p["fwd_list"])
    followed = 0
    for i in np.flatnonzero(c["event"][:n] == F.NEW_CONNECTION):
        l = int(p["fwd_list"][i])
        if rb[l] >= 0 and rb[rb[l]] >= 0:
            end = l
            while rb[end] >= 0:
                end = int(rb[end])
            assert c["alive"][end] and c["kp_lm"][1][c["best_idx"][i]] == end
            followed += 1
    assert followed >= 1
    # a survivor that gained target 2 as observer THROUGH A MERGE at target 1 is no query at target 2: alive, a duplicate row at target 1,
    # target 2's observer in its final list and not in its initial one, no connection of its own at target 2
    p, c, i = results["basic"]
    n, t = len(p["fwd_list"]), p["table"]
    o2 = p["keyframes"][2]["observer"]
    has = lambda tab, cnt, l: o2 in tab["obs_observer"][t["obs_off"][l]:t["obs_off"][l] + cnt[l]]  # noqa: E731
    rows = [r for r in range(n) if c["event"][r] == F.DUP_SURVIVED and c["alive"][p["fwd_list"][r]] and has(c, c["obs_cnt"], p["fwd_list"][r])
            and not has(t, t["obs_cnt"], p["fwd_list"][r]) and c["event"][n + r] == F.NONE]
    assert rows and all(c["best_idx"][n + r] < 0 for r in rows) and any(i["best_idx"][n + r] >= 0 for r in rows)
    # a crowded cell: 64 and 65 keypoints around one reprojection
    for name, k in (("cell64", 63), ("cell65", 64)):
        assert len(results[name][0]["keyframes"][1]["xy"]) == 60 + 40 + k


def test_the_overflow_class_overflows():
    p = F.prepared("overflow")
    with pytest.raises(F.Overflow):
        F.cpu_chain(p)


def test_entry_point_refuses_null_arguments_without_a_device():
    from stella_vslam_amd import _lib
    L = _lib.lib()
    assert L.svgpu_fuse_landmarks_batch(None, 1, None, 0, None, None, None, 0, None, 0, None, 8, None, None, 0.2, 0.3, 3.0, 1, None, None, None, None) == 1
