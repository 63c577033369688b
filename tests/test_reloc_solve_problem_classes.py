"""The classes of tests/reloc_solve_problems.py reach the status values they are named for -- shown on the CPU with the existing restatements
only (tests/pnp_problems.find_via_ransac, the oracle's pose optimiser and projection matcher behind RP.compose_single_calls) -- so the GPU
test cannot pass by never leaving one branch.  Reached: PnP failed (too few matches, and no hypothesis with enough inliers), optimise
failed, the count failure of the first and of the second stage, the final count failure (with one stage), accepted, inactive.  Not reached
by a scene: the final failure of a two-stage chain (see the builder's docstring for why).  Also here: the host check of the call's
scratch layout, and the header / binding agreement on the entry point."""
import pathlib
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import host_check
from tests import pnp_problems as PP
from tests import reloc_refine_problems as RP
from tests import reloc_solve_problems as SP
from tests.test_reloc_refine_problem_classes import oracle_backend

ROOT = pathlib.Path(__file__).resolve().parent.parent


def cpu_backend():
    def do_pnp(p, brg, pos, octv, samples):
        r = PP.find_via_ransac(np.asarray(brg), np.asarray(pos), octv, p["scale_factors"], samples, p["min_num_inliers"], bool(p["recompute"]),
                               p["gauss_newton_num_iter"])
        pose = np.concatenate([r["R"], r["t"][:, None]], 1).reshape(12) if r["valid"] else np.zeros(12)
        return int(r["valid"]), pose, r["is_inlier"].astype(np.uint8), r["best_iter"]

    def do_opt(p, pose, pos_w, uvr, w, hb):
        if len(pos_w) < 5:  # pose_optimizer_g2o.cc:109-111
            return 0, pose, np.zeros(len(pos_w), np.uint8), 0
        nv, out, flags, _ = O.pose_optimize(pose, pos_w, uvr, w, hb, p["intrinsics"], p["num_trials_robust"], p["num_trials"], p["num_each_iter"],
                                            reset_flag_each_round=bool(p["reset_stop_flag_each_round"]))
        return nv, out, flags, 0

    def do_refine(one):
        return RP.compose_single_calls(one, oracle_backend(one))
    return do_pnp, do_opt, do_refine


@pytest.fixture(scope="module")
def results():
    P = SP.classes()
    return P, {name: SP.chain(p, cpu_backend()) for name, p in P.items()}


def test_every_class_reaches_its_status(results):
    P, R = results
    for name, r in R.items():
        assert r["status"].tolist() == SP.EXPECT[name], (name, r["status"], r["opt_num_valid"], r["num_found"], r["num_valid"])
    seen = {s for r in R.values() for s in r["status"].tolist()}
    assert {-1, 0, 1, 2, SP.PNP_FAILED, SP.OPTIMIZE_FAILED} <= seen
    assert R["one_stage"]["status"][1] == 1 + P["one_stage"]["num_stages"]  # the final count failure
    assert R["each_status"]["status"][5] == 2 and P["each_status"]["num_stages"] == 2  # the second stage's count failure


def test_the_branches_are_taken_for_the_reason_named(results):
    P, R = results
    e, p = R["each_status"], P["each_status"]
    n = np.diff(p["match_off"])
    assert n[1] < p["min_num_inliers"] and not e["pnp_valid"][1]              # launches nothing
    assert n[2] >= 30 and not e["pnp_valid"][2] and e["best_iter"][2] == -1    # ran, no hypothesis wins
    assert e["pnp_valid"][3] and 5 <= e["opt_num_valid"][3] <= SP.MIN_OPT - 3  # optimised, below its threshold
    m = p["min_num_valid_obs"]
    assert e["opt_num_valid"][4] >= SP.MIN_OPT + 3 and e["opt_num_valid"][4] + e["num_found"][4, 0] <= m - 5
    assert e["opt_num_valid"][5] + e["num_found"][5, 0] >= m + 5 and e["num_valid"][5, 0] + e["num_found"][5, 1] <= m - 5
    # PnP outliers exist and are not optimised; matches name keyframe entries and neighbours' landmarks
    a, pa = R["accepted"], P["accepted"]
    assert (a["is_inlier"] == 0).sum() >= 5 * 5 and not a["opt_outlier"][a["is_inlier"] == 0].any()
    assert (pa["m_kf_entry"] >= 0).sum() >= 50 and (pa["m_kf_entry"] < 0).sum() >= 20
    assert (a["opt_num_valid"] >= SP.MIN_OPT + 5).all() and (a["num_found"][:, 0] >= 50).all()
    # an entry a held match names is spent: the stages do not match it again
    for c in range(pa["num_candidates"]):
        lo, hi = pa["match_off"][c], pa["match_off"][c + 1]
        held = (a["is_inlier"][lo:hi] != 0) & (a["opt_outlier"][lo:hi] == 0) & (pa["m_kf_entry"][lo:hi] >= 0)
        assert held.sum() >= 20 and (a["match_kf"][pa["kf_off"][c] + pa["m_kf_entry"][lo:hi][held]] == -1).all()
    xr = P["stereo"]["t_xright"]
    assert 0 < (xr >= 0).sum() < len(xr)


def test_scene_sizes_and_sub_problems():
    P = SP.classes()
    for name, p in P.items():
        assert 300 <= p["nt"] <= 600 and p["num_levels"] == 8 and 8 <= p["num_iter"] <= 16 and 1 <= p["num_candidates"] <= 7, name
        for c in range(p["num_candidates"]):
            k = p["m_keypt"][p["match_off"][c]:p["match_off"][c + 1]]
            assert (np.diff(k) > 0).all()
    p = P["each_status"]
    q = SP.sub(p, [5, 0])
    assert q["num_candidates"] == 2 and np.array_equal(q["m_pos_w"], p["m_pos_w"][SP.match_rows(p, [5, 0])])
    assert np.array_equal(q["samples"][0], p["samples"][5]) and np.array_equal(q["pos_w"], p["pos_w"][RP.rows_of(p, [5, 0])])


def test_reloc_solve_arena_layout(tmp_path):
    out = host_check.build_and_run("reloc_solve_arena_check.cpp", "reloc solve arena ok", tmp_path)
    assert out.count("ok K ") == 6, out


def test_header_declares_the_entry_point_and_the_binding_reads_it():
    from stella_vslam_amd import _lib
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    assert re.search(r"^int\s+svgpu_reloc_solve_batch\s*\(", hdr, flags=re.M)
    restype, argtypes = _lib.parse_header(hdr)["svgpu_reloc_solve_batch"]
    assert len(argtypes) == 60
    assert re.search(r"#define SVGPU_RELOC_PNP_FAILED \(-2\)", hdr) and re.search(r"#define SVGPU_RELOC_OPTIMIZE_FAILED \(-3\)", hdr)
