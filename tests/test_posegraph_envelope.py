"""CPU tests of the pose graph's direct solver: the envelope planner and the plain fp64 elimination
(stella_vslam_amd/csrc/posegraph_envelope_plan.h) through tests/posegraph_envelope_check.cpp, built with g++ against that header alone
(the solver's scratch layout is checked with the other layouts, in tests/test_arena_layouts.py).
The envelopes of the natural and of the interleaved order are computed here, independently, and handed to the check program: the
planner's choice may not be larger than either."""
import pytest

from tests import posegraph_envelope_graphs as G
from tests import posegraph_problems as T

GRAPHS = {
    "one free vertex": lambda: (1, [(0, -1), (-1, 0)]),
    "chain of 8": lambda: G.chain(8, 1, loop=False),
    "ring of 63": lambda: G.ring(63),
    "ring of 64": lambda: G.ring(64),
    "ring of 65": lambda: G.ring(65),
    "class e": lambda: G.from_problem(T.problem("e-fs0")),
    "hub of 40": lambda: G.hub(40),
    "duplicates in both orientations": G.duplicates,
    "two components": G.two_components,
    "chain of 2049 with a far loop pair": lambda: G.chain(2049, 3),
    "every pair of 70": lambda: G.dense(70),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_plan_invariants_and_host_elimination(name):
    nfree, edges = GRAPHS[name]()
    rc, out, info = G.run_check(nfree, edges)
    print(f"{name}: {info}")
    assert rc == 0, out
    assert "envelope plan ok" in out and "FAIL" not in out
    assert info["blocks"] <= min(info["natural"], info["interleaved"])
    assert info["residual"] <= 1e-12


def test_class_e_loses_its_fixed_vertices_and_is_banded():
    nfree, edges = G.from_problem(T.problem("e-fs0"))
    assert nfree == 297 and any(a < 0 or b < 0 for a, b in edges)
    _, _, info = G.run_check(nfree, edges)
    assert info["blocks"] < 297 * 12 and info["max_column_rows"] <= 12   # a band plus the few long rows of the loop edges


def test_one_long_row_beats_a_wider_band_on_the_chain_of_2049():
    """The far loop pair costs the natural order ONE row of 2 049 blocks; the interleaved order pays a band twice as wide everywhere."""
    _, _, info = G.run_check(*G.chain(2049, 3))
    assert info["natural"] == 4 * 2049 - 6 + 2049 - 4 and info["blocks"] <= info["natural"] < info["interleaved"]

