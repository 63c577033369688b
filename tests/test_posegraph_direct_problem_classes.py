"""CPU test of the planted classes of the direct solver's tests (tests/posegraph_direct_problems.py): every class passes, in the fp64 and
in the long double form of the restatement, the decision filter tests/test_posegraph_problem_classes.py applies -- the two forms take
the same decisions and end within 1e-3 of each other, every gain stays 1e-5 away from the threshold and every |rho| above 1e-6 -- so
that an implementation that differs by rounding takes the same decisions."""
import numpy as np
import pytest

from tests import posegraph_direct_problems as D
from tests import posegraph_envelope_graphs as G
from tests import posegraph_problems as T


@pytest.mark.parametrize("case", D.CASES)
def test_two_forms_agree_and_pass_the_decision_filter(case):
    a, b = D.solved(case, "fp64"), D.solved(case, "ld")
    dev = T.deviation(a["sim3"], b["sim3"])
    print(f"{case}: LM {a['lm_iterations']} trials {a['lm_trials']} gain {a['stopped_by_gain']} chi2 {a['initial_chi2']:.3e} -> {a['final_chi2']:.6e} two-form deviation {dev:.2e}")
    assert (a["lm_iterations"], a["lm_trials"], a["stopped_by_gain"]) == (b["lm_iterations"], b["lm_trials"], b["stopped_by_gain"])
    assert a["lm_iterations"] >= 1
    assert dev <= 1e-3
    for r in (a, b):
        for gain in r["gains"]:
            assert abs(gain - T.GAIN_THR) > 1e-5
        for rho, _, _ in r["rhos"]:
            assert abs(rho) > 1e-6


def test_the_classes_hold_what_they_are_named_for():
    k = D.problem("k-fs0")
    pairs = list(zip(k["e1"].tolist(), k["e2"].tolist()))
    assert pairs.count((2, 1)) == 3 and pairs.count((1, 2)) == 1
    l = D.problem("l-fs0")
    nfree, edges = G.from_problem(l)
    slot4 = 4 - 2  # vertices 0 and 3 are fixed in front of it
    assert nfree == 5 and all(b < 0 for a, b in edges if a == slot4) and all(a < 0 for a, b in edges if b == slot4)
    m = D.problem("m-fs0")
    assert int((m["e2"] == 1).sum()) == 40 and len(m["e1"]) == 81
    n = D.problem("n-fs0")
    assert len(n["sim3"]) == 130 and n["fixed"][65] == 1 and n["fixed"].sum() == 1 and (126, 3) in list(zip(n["e1"].tolist(), n["e2"].tolist()))
    o = D.problem("o-fs0")
    assert o["fixed"].sum() == 2 and not np.any((o["e1"] < 8) != (o["e2"] < 8))
