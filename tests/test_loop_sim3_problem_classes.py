"""The problem classes of tests/loop_sim3_problems.py are what they claim to be, shown on the CPU by the numpy restatement of the scale alone
(module/loop_detector.cc:540-573): the number of kept ratios per candidate, the candidates that end without a scale, and where the planted
boundary pairs sit."""
import pathlib
import re

import numpy as np
import pytest

from tests import loop_sim3_problems as LP

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def problems():
    return LP.classes()


@pytest.fixture(scope="module")
def scale_problems():
    return LP.scale_classes()


def test_every_class_keeps_the_ratios_its_knobs_plant(problems):
    for name, p in problems.items():
        for c in range(p["num_candidates"]):
            s, kept, idx = LP.scale_restatement(p, c)
            assert len(kept) == LP.planted_kept(p, c), (name, c)
            assert (kept > 0).all() and np.isfinite(kept).all()
            if len(kept):
                assert abs(float(s) - 1.05) < 2e-3 or name == "stereo_fix_scale", (name, c, s)
                assert (p["prior_state"][c][idx] == 1).all() and (p["has_lm1"][idx] != 0).all()


def test_no_scale_is_reached_where_the_class_says(problems):
    for name, want in LP.EXPECT.items():
        p = problems[name]
        if p["scale_12_in"] is not None:
            continue
        for c, st in enumerate(want):
            assert (LP.scale_restatement(p, c)[0] is None) == (st == LP.NO_SCALE or (st == -1 and LP.planted_kept(p, c) == 0)), (name, c)
    # without priors there is no ratio: the class runs on scale_12_in
    p = problems["no_priors"]
    assert p["scale_12_in"] is not None and all(LP.scale_restatement(p, c)[0] is None for c in range(p["num_candidates"]))
    # erased and swung priors give none, unindexed ones do
    assert LP.planted_kept(problems["prior_erased"], 1) == 0 and (problems["prior_erased"]["prior_state"][1] == 2).sum() == 60
    q = problems["prior_unindexed"]
    assert ((q["prior_state"][1] == 1) & (q["has_lm1"] != 0)).sum() == 70 and len(LP.scale_restatement(q, 1)[1]) == 60
    assert ((q["prior_state"][0] == 1) & (q["prior_idx2"][0] < 0)).sum() == 60


def test_shapes_are_what_the_gpu_test_relies_on(problems):
    n2 = np.diff(problems["unequal"]["kf2_off"]).tolist()
    assert n2 == [0, 1, 150, 400]
    m = problems["many_tiny"]
    assert m["num_candidates"] == 40 and np.diff(m["kf2_off"]).max() <= 30
    assert problems["each_status"]["active"].tolist() == [1, 1, 1, 0]
    ls = problems["long_sets"]
    sets = np.concatenate([ls["kf2_off"], [ls["kf2_off"][-1] + ls["n1"]]]).tolist()  # the binning's keypoint sets: the candidates, then keyframe 1
    assert sets == [0, 300, 1600, 2700] and sets[1] % 256 and sets[2] % 256 and sets[2] - sets[1] > 1024
    assert {c["model"] for c in problems["mixed_models"]["cam2"]} == {0, 1, 2} and problems["mixed_models"]["cam1"]["model"] == 0
    t = problems["twins"]
    assert all(np.array_equal(t[k][0], t[k][1]) for k in LP.PER_CAND)
    for name, p in problems.items():
        assert (p["prior_idx2"] < np.diff(p["kf2_off"])[:, None]).all(), name
        q = p["sim3_12"][:, :4]
        assert np.abs((q * q).sum(1) - 1.0).max() < 1e-12, name


def _first_best(lists, q_desc, t_desc, n):
    """the matcher pass on restated lists: the first listed keypoint at the smallest Hamming distance, if within 100 bits"""
    out = np.full(n, -1, np.int32)
    for i, got in lists.items():
        d = [int(np.unpackbits(q_desc[i] ^ t_desc[k]).sum()) for k, _ in got]
        if d and min(d) <= 100:
            out[i] = got[int(np.argmin(d))][0]
    return out


def test_cell_order_ties_are_decided_by_the_order_of_the_lists(problems):
    """A condition on the inputs: in both passes at least 8 rows reach their best Hamming distance at two or more of the keypoints the
    window lists, some of them inside one cell (index order decides) and some across the two cells (column-major order decides).  The
    lists are the numpy restatement's (window_lists), which is itself held to the CPU oracle's matcher here."""
    from oracle import oracle as O
    p = problems["cell_order"]
    assert p["num_candidates"] == 2 and p["n1"] == 64 and np.diff(p["kf2_off"]).tolist() == [40, 40]
    cell = lambda xy: set((np.floor(xy[:, 0] / LP.CELL_W).astype(int) * LP.GRID_ROWS + np.floor(xy[:, 1] / LP.CELL_H).astype(int)).tolist())
    cam1 = LP.oracle_camera(p["cam1"])
    assert (cam1.min_x, cam1.max_x, cam1.min_y, cam1.max_y) == (0.0, LP.WIDTH, 0.0, LP.HEIGHT)  # what window_lists takes the grid's bounds to be
    c1 = sorted(cell(p["xy1"]))
    assert len(c1) == 2 and c1[1] - c1[0] == LP.GRID_ROWS  # two cells, neighbours in x
    tied = dict(A_inside=0, A_across=0, B_inside=0, B_across=0)
    for c in range(2):
        lo, hi = int(p["kf2_off"][c]), int(p["kf2_off"][c + 1])
        sl = lambda k: p[k][lo:hi]
        c2 = sorted(cell(sl("xy2")))
        assert len(c2) == 2 and c2[1] - c2[0] == LP.GRID_ROWS, c
        A, B = LP.window_lists(p, c)
        ia, aa = LP.best_distance_ties(A, p["lm_desc1"], sl("desc2"))
        ib, ab = LP.best_distance_ties(B, sl("lm_desc2"), p["desc1"])
        tied["A_inside"] += len(ia)
        tied["A_across"] += len(aa)
        tied["B_inside"] += len(ib)
        tied["B_across"] += len(ab)
        # the restated lists give the oracle's matches, ties included
        state, pidx = p["prior_state"][c], p["prior_idx2"][c]
        b1 = (state != 0) & (pidx >= 0)
        b2 = np.zeros(hi - lo, bool)
        b2[pidx[b1]] = True
        kf1 = dict(pos_w=p["pos_w1"], valid=((p["has_lm1"] != 0) & ~b1).astype(np.uint8), min_valid_dist=p["min_valid1"], max_valid_dist=p["max_valid1"],
                   lm_desc=p["lm_desc1"], desc=p["desc1"], xy=p["xy1"], octave=p["octave1"])
        kf2 = dict(pos_w=sl("pos_w2"), valid=((sl("has_lm2") != 0) & ~b2).astype(np.uint8), min_valid_dist=sl("min_valid2"), max_valid_dist=sl("max_valid2"),
                   lm_desc=sl("lm_desc2"), desc=sl("desc2"), xy=sl("xy2"), octave=sl("octave2"))
        T1, T2, cc = p["pose_1w"].reshape(3, 4), p["pose_2w"][c].reshape(3, 4), np.ascontiguousarray
        m21, m12, _, _ = O.match_keyframes_mutually(cam1, LP.oracle_camera(p["cam2"][c]), cc(T1[:, :3]), cc(T1[:, 3]), cc(T2[:, :3]), cc(T2[:, 3]),
                                                    float(LP.scale_restatement(p, c)[0]), p["rot_12"][c], p["trans_12"][c], kf1, kf2, p["scale_factors"],
                                                    p["log_scale_factor"], float(p["margin"]))
        assert np.array_equal(_first_best(A, p["lm_desc1"], sl("desc2"), p["n1"]), m21), c
        assert np.array_equal(_first_best(B, sl("lm_desc2"), p["desc1"], hi - lo), m12), c
    print(tied)
    assert tied["A_inside"] + tied["A_across"] >= 8 and tied["B_inside"] + tied["B_across"] >= 8, tied
    assert min(tied.values()) >= 2, tied


def test_scale_classes_count_tie_and_cross_the_workgroup(scale_problems):
    for name, want in LP.SCALE_KEPT.items():
        s, kept, _ = LP.scale_restatement(scale_problems[name], 0)
        assert len(kept) == want, name
        assert s == np.sort(kept)[(want - 1) // 2]
    assert scale_problems["kept_1025"]["n1"] == 1100
    _, kept, _ = LP.scale_restatement(scale_problems["ties"], 0)
    vals, counts = np.unique(kept, return_counts=True)
    assert counts.max() == 6  # six pairs share one ratio, and the median is among them or beside them
    # kept_2: the lower of the two ((2 - 1) / 2 = 0)
    s, kept, _ = LP.scale_restatement(scale_problems["kept_2"], 0)
    assert s == kept.min()


def test_boundary_pairs_sit_on_the_threshold_and_one_float_above(scale_problems):
    p = scale_problems["boundary"]
    at, above = p["boundary_idx"]
    cos = lambda i: LP.cos_and_ratio(p["pose_1w_in_cand"][0], p["pose_1w"], p["prior_pos_w"][0, i], p["pos_w1"][i])[0][0]
    assert cos(at) == LP.COS_THR and cos(above) == np.nextafter(LP.COS_THR, np.float32(2.0))
    _, kept, idx = LP.scale_restatement(p, 0)
    assert at not in idx and above in idx  # strict: the pair on the threshold is rejected
    assert ((p["prior_state"][0] == 1) & (p["has_lm1"] != 0)).sum() == 5 and len(kept) == 4


def test_header_declares_the_entry_point_and_the_binding_reads_it():
    from stella_vslam_amd import _lib
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    assert re.search(r"^int\s+svgpu_loop_sim3_batch\s*\(", hdr, flags=re.M)
    restype, argtypes = _lib.parse_header(hdr)["svgpu_loop_sim3_batch"]
    assert len(argtypes) == 58
