"""CPU tests of the pose-graph yardstick (tests/posegraph_problems.py) and of the host edge builder.

1. The two forms of the restatement (fp64 with LAPACK, long double with a hand-written Cholesky) take the same decisions on every planted
   case and end within 1e-3 of each other (the planted corrections are 1e-2 .. 1; the numeric Jacobians' noise of about 1e-7 times the
   condition of the damped systems, up to 4.4e8 on class e, stays far below that).
2. The decision filter: in both forms every gain stays 1e-5 away from the threshold 1e-3 and every rho 1e-6 away from 0, so that an
   implementation that differs by rounding takes the same decisions.  One exception is admitted and checked as such: class (h), where
   chi2 before and after the step is EXACTLY zero and rho is therefore exactly 0 in any implementation (no rounding can move it).
   Under the restated rule (oracle/ba_oracle.c: `rho == 0` ends the optimisation) that class ends after its first iteration without the
   gain rule being consulted.  Class (j) is its counterpart with small non-zero errors: it stays inside the small branches of log and
   ends by the gain rule.  Class (a) holds its free vertex by two disagreeing edges, because a single edge can be satisfied exactly and
   the run would then end in rounding noise.
3. build_pose_graph_edges (stella_vslam_amd/host/drop_in/graph_optimizer_hip.cc) against a Python transcription of the four edge loops
   of optimize/graph_optimizer.cc:127-250 on hand-built graphs."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from tests import posegraph_problems as T

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("case", T.CASES)
def test_two_forms_agree_and_pass_the_decision_filter(case):
    a, b = T.solved(case, "fp64"), T.solved(case, "ld")
    dev = T.deviation(a["sim3"], b["sim3"])
    print(f"{case}: LM {a['lm_iterations']} trials {a['lm_trials']} gain {a['stopped_by_gain']} chi2 {a['initial_chi2']:.3e} -> {a['final_chi2']:.6e} two-form deviation {dev:.2e}")
    assert (a["lm_iterations"], a["lm_trials"], a["stopped_by_gain"]) == (b["lm_iterations"], b["lm_trials"], b["stopped_by_gain"])
    assert a["lm_iterations"] >= 1
    assert dev <= 1e-3
    for r in (a, b):
        for gain in r["gains"]:
            assert abs(gain - T.GAIN_THR) > 1e-5
        for rho, chi_before, chi_after in r["rhos"]:
            if case.startswith("h-"):
                assert rho == 0.0 and chi_before == 0.0 and chi_after == 0.0
            else:
                assert abs(rho) > 1e-6


def test_class_h_does_not_move():
    for case in ("h-fs0", "h-fs1"):
        p, r = T.problem(case), T.solved(case, "fp64")
        assert np.array_equal(np.asarray(r["sim3"], np.float64), p["sim3"])
        assert (r["lm_iterations"], r["lm_trials"], r["initial_chi2"], r["final_chi2"]) == (1, 1, 0.0, 0.0)


def test_class_j_stays_in_the_small_branches_and_ends_by_the_gain_rule():
    for case in ("j-fs0", "j-fs1"):
        p, r = T.problem(case), T.solved(case, "fp64")
        e = T.edge_errors(p["sim3"], dict(p, _meas=p["meas"]))
        theta = np.sqrt((e[:, :3] ** 2).sum(1))
        assert 0 < np.abs(e[:, 6]).max() < T.EPS and np.cos(theta).min() > 1 - T.EPS and theta.max() > 1e-4
        assert r["stopped_by_gain"] == 1 and r["final_chi2"] > 0


def test_large_branches_are_met_in_class_i():
    p = T.problem("i-fs0")
    e = T.edge_errors(p["sim3"], dict(p, _meas=p["meas"]))
    assert np.abs(e[:, :3]).max() > 1.4 and abs(e[:, 6]).max() > 0.69  # near pi / 2; log 2


# ------------------------------------------------------------------------------------------------ build_pose_graph_edges
_transcription = T.transcribe_edges


def _hand_built_graph():
    rng = np.random.default_rng(5)
    S = T._trajectory(rng, 10)
    corr = T.make_sim3(np.array([0.02, -0.01, 0.03]), np.array([0.1, 0.2, -0.1]), 1.05)
    ids = [0, 2, 3, 5, 4, 7, 8, 9, 11, 12]               # keyframe 4 is a child of 5: a child with id < its parent's
    parent = {0: -1, 2: 0, 3: 2, 5: 3, 4: 5, 7: 5, 8: 7, 9: 8, 11: 9, 12: 11}
    kfs = [dict(id=i, erased=0, parent=parent[i], loop=[], covis=[], cw=S[k], non=None) for k, i in enumerate(ids)]
    by = {k["id"]: k for k in kfs}

    def covis(a, b, w):
        by[a]["covis"].append((b, w))
        by[b]["covis"].append((a, w))
    covis(12, 11, 200), covis(12, 9, 150), covis(12, 2, 120), covis(11, 3, 110), covis(11, 8, 105), covis(9, 7, 130), covis(8, 5, 140)
    covis(9, 3, 125), covis(7, 3, 135), covis(12, 3, 60), covis(4, 3, 300), covis(7, 4, 160), covis(11, 2, 50), covis(8, 2, 115)
    by[9]["loop"], by[3]["loop"] = [3], [9]               # an earlier loop edge: the covisibility 9 - 3 is also a loop edge
    by[8]["erased"] = 1                                  # an erased neighbour of 11, above the threshold
    for k in kfs:
        k["covis"].sort(key=lambda c: -c[1])
    for i in (12, 11):                                   # the current keyframe and its neighbour were pre-corrected
        by[i]["non"] = by[i]["cw"]
        by[i]["cw"] = T.sim3_mul(corr, by[i]["cw"])
    # loop connections: curr 12 -> loop 2 holds whatever its weight; 12 -> 3 is below the threshold (60) and is dropped; 11 -> 3 (110)
    # holds and is then found "already inserted" by the covisibility loop; 11 -> 2 (50) is dropped
    conns = [(11, [2, 3]), (12, [2, 3])]
    return kfs, conns, 12, 2, 100


def _write_graph(path, kfs, conns, curr_id, loop_id, min_shared):
    out = [f"{len(kfs)} {curr_id} {loop_id} {min_shared}"]
    f = lambda v: " ".join(repr(float(x)) for x in v)
    for k in kfs:
        non = k["non"] if k["non"] is not None else np.zeros(8)
        out.append(f"{k['id']} {k['erased']} {k['parent']} {int(k['non'] is not None)} {f(k['cw'])} {f(non)} {len(k['loop'])} "
                   + " ".join(str(i) for i in k["loop"]) + f" {len(k['covis'])} " + " ".join(f"{i} {w}" for i, w in k["covis"]))
    out.append(str(len(conns)))
    for i, ids in conns:
        out.append(f"{i} {len(ids)} " + " ".join(str(j) for j in ids))
    path.write_text("\n".join(out) + "\n")


def test_build_pose_graph_edges_against_the_transcription(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/posegraph_edges_check.cpp")
    exe = tmp_path / "posegraph_edges_check"
    host = ROOT / "stella_vslam_amd" / "host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-DSVGPU_POSE_GRAPH_EDGES_ONLY", "-I", str(host), "-I", str(ROOT / "stella_vslam_amd" / "csrc"),
                           str(ROOT / "tests" / "posegraph_edges_check.cpp"), str(host / "drop_in" / "graph_optimizer_hip.cc"), "-o", str(exe)])
    kfs, conns, curr_id, loop_id, min_shared = _hand_built_graph()
    exp = _transcription(kfs, conns, curr_id, loop_id, min_shared)
    pairs = [(a, b) for a, b, _ in exp]
    # the hand-built cases are really there
    assert (12, 2) in pairs and (12, 3) not in pairs and (11, 2) not in pairs      # curr -> loop below the threshold stays; the others go
    assert pairs.count((11, 3)) == 1                                               # inserted by loop_connections, not again as a covisibility
    assert (9, 3) in pairs and pairs.count((9, 3)) == 1                            # the loop edge, not repeated as a covisibility
    assert not any(a == 4 for a, _ in pairs)                                       # a child below its parent's id adds nothing at all
    assert (7, 4) in pairs                                                         # ... but its neighbours still reach it
    assert (11, 8) not in pairs and (8, 5) in pairs                                # an erased keyframe is skipped as a neighbour only
    assert (7, 3) in pairs and (8, 7) in pairs and (12, 9) in pairs
    graph = tmp_path / "graph.txt"
    _write_graph(graph, kfs, conns, curr_id, loop_id, min_shared)
    r = subprocess.run([str(exe), str(graph)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert [(int(g[0]), int(g[1])) for g in got] == pairs
    for g, (_, _, m) in zip(got, exp):
        assert np.abs(np.array(g[2:], np.float64) - m).max() <= 1e-14
