"""The planted brute-force problems (tests/bf_problems.py) do what they claim on the CPU oracle: the planted distances hold, every class
drives the branch it is named after, and O.brute_force_match equals the literal Python loop (tests/test_oracle_match.py) on every case."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import bf_problems as BP
from tests.test_oracle_match import py_brute_force


@pytest.fixture(scope="module")
def classes():
    return BP.all_classes()


def _row(case, j):
    """the target query j took, or -1"""
    exp = case.oracle()
    hit = np.flatnonzero(exp == j)
    return int(hit[0]) if len(hit) else -1


def test_threshold_class_matches_at_50_never_at_51(classes):
    for case in classes["threshold"]:
        D = O.hamming_matrix(case.d1, case.d2)
        got = {b: [] for b in (49, 50, 51)}
        for j, (i, b) in case.info["best"].items():
            assert D[j, i] == b
            assert np.delete(D[j], i).min() >= 67
            got[b].append(_row(case, j) == i)
        assert all(got[49]) and all(got[50]) and not any(got[51]), (case.name, got)


def test_ratio_equality_class_accepts_equality_and_rejects_one_ulp_below(classes):
    seen = set()
    for case in classes["ratio_equality"]:
        i, j = case.info["target"], case.info["query"]
        b, s = case.info["best"], case.info["second"]
        D = O.hamming_matrix(case.d1, case.d2)
        assert D[j, i] == b and sorted(D[j])[1] == s
        assert (_row(case, j) == i) == case.info["accept"], case.name
        if case.info["tag"] == "eq":
            assert np.float32(case.ratio) * np.float32(s) == np.float32(b) and case.info["accept"]
        seen.add((case.info["tag"], case.info["accept"]))
    # equality accepted, one ulp above accepted, one ulp below rejected (for every tuple here: the products leave best)
    assert seen == {("eq", True), ("up", True), ("down", False)}


def test_around_dmax_class_plants_seconds_at_the_cutoff(classes):
    cases = classes["around_dmax"]
    cut = {c.ratio: c.info["dmax"] for c in cases if c.name.startswith("dmax_")}
    assert cut == {0.5: 102, 0.6: 85, 0.75: 68, 0.8: 64, 1.0: 52, 1.5: 50}
    for case in cases:
        if not case.name.startswith("dmax_"):
            continue
        D = O.hamming_matrix(case.d1, case.d2)
        offs = set()
        for j, (s, b) in case.info["planted"].items():
            row = np.sort(D[j])
            assert row[0] == b and row[1] == s
            offs.add(s - case.info["dmax"])
            assert (_row(case, j) >= 0) == BP.accepts(b, s, case.ratio)
        assert offs == {0, 1, 2}
    # the kernel switch: 0.40 -> dmax 127 (< 128: the MFMA kernel) with over-full rows, 0.39 -> 130; 0, negative, NaN -> 256
    by = {c.name: c for c in cases}
    assert by["ratio_0.4"].info["dmax"] == 127 and by["ratio_0.39"].info["dmax"] == 130
    assert all(by[n].info["dmax"] == 256 for n in ("ratio_0.0", "ratio_-0.5", "ratio_nan"))
    c = by["ratio_0.4"]
    assert ((O.hamming_matrix(c.d1, c.d2) <= 127).sum(1) > 16).mean() > 0.9  # nearly every row overflows 16 slots
    # degenerate ratios: 0 and negative only ever accept best == 0 (with the second at 0 too when negative); NaN accepts any best <= 50
    D = O.hamming_matrix(c.d1, c.d2)
    for name in ("ratio_0.0", "ratio_-0.5", "ratio_nan"):
        exp = by[name].oracle()
        i = np.flatnonzero(exp >= 0)
        best = D[exp[i], i]
        assert len(i) > 0
        if name == "ratio_nan":
            assert best.max() > 0 and len(i) > (by["ratio_0.4"].oracle() >= 0).sum()
        else:
            assert (best == 0).all()


def test_ties_class(classes):
    by = {c.name: c for c in classes["ties"]}
    c = by["tie_bins"]
    exp = c.oracle()
    bins = np.floor(c.a1).astype(int)
    for j, w in c.info["winner"].items():
        assert exp[w] == j
        tied = np.flatnonzero(O.hamming_matrix(c.d1, c.d2)[j] == 20)
        assert len(tied) == 5 and w == tied.min() and bins[w] != bins[tied].min()  # the winner is not first in angle order
    c = by["tie_over16_r1.0"]
    assert (O.hamming_matrix(c.d1, c.d2)[2] == 30).sum() == 20
    assert _row(c, 2) == c.info["lowest"] and _row(by["tie_over16_r0.75"], 2) == -1
    # d_beyond: the listed 16 are claimed first; the 17th (unlisted, at the same distance) decides
    for name in ("tie_beyond_full_row", "tie_beyond_ratio"):
        c = by[name]
        exp = c.oracle()
        t = c.info["t"]
        assert [int(exp[i]) for i in t[:16]] == list(range(16))
        assert (exp[t[16]] == 16) == c.info["match16"] and (exp == 16).sum() == int(c.info["match16"])
    for name in ("all_identical_r0.75", "all_identical_r0.3"):
        assert np.array_equal(by[name].oracle(), np.arange(300))


def test_popcount_class_hits_the_piece_boundaries(classes):
    c = classes["popcount"][0]
    pops = set(BP.popcount(c.d1).tolist()) & set(BP.popcount(c.d2).tolist())
    assert {0, 1, 127, 128, 254, 255, 256} <= pops
    z = classes["popcount"][3]
    assert (BP.popcount(z.d2) <= 1).all() and BP.popcount(z.d1).max() < 60
    for case in classes["popcount"]:
        assert (case.oracle() >= 0).sum() > 0 or case.ratio < 1.0


def test_orientation_class_gate_decides(classes):
    n = 0
    for case in classes["orientation"]:
        D = O.hamming_matrix(case.d1, case.d2)
        assert D[1, 23] == 10 and D[1, 5] == 30
        exp = case.oracle()
        assert (exp[23] == 1) == case.info["kept"], case.name
        n += not case.info["kept"]
    assert n >= 6
    by = {c.name: c for c in classes["orientation"]}
    # exactly 30 apart is kept, the next float beyond is not
    assert by["gate_10.0_40.0/ori1"].info["kept"] and not by[f"gate_10.0_{BP._nx(40.0, 99)!r}/ori1"].info["kept"]
    assert by["gate_360.0_30.0/ori1"].info["kept"] and by["gate_0.0_330.0/ori1"].info["kept"]
    # NaN angles are never gated; a query angle <= -500 is an ordinary angle
    assert by["gate_nan_10.0/ori1"].oracle()[23] == 1 and by["gate_10.0_nan/ori1"].oracle()[23] == 1
    assert by["gate_-1000.0_-1000.0/ori1"].oracle()[23] == 1 and by["gate_-600.0_10.0/ori0"].oracle()[23] == 1


def test_domino_class_shifts_every_query_by_one(classes):
    for case in classes["domino"]:
        n = len(case.d1)
        D = O.hamming_matrix(case.d1, case.d2)
        j = np.arange(1, n)
        assert D[0, 0] == 10 and (D[j, j - 1] == 10).all() and (D[j, j] == 11).all()
        assert (np.argmin(D, 1)[1:] == j - 1).all()  # every later query's first choice is the target its predecessor takes
        assert np.array_equal(case.oracle(), np.arange(n))
        # without the claims, the ratio test rejects every q_j (j >= 1): 0.75 * 11 < 10
        assert not BP.accepts(10, 11, case.ratio)


def test_valid2_class(classes):
    by = {c.name: c for c in classes["valid2"]}
    full = by["valid2_none"].oracle()
    assert (full >= 0).sum() > 50 and np.array_equal(by["valid2_ones"].oracle(), full)
    assert (by["valid2_zero"].oracle() == -1).all()
    alt = by["valid2_alternating"].oracle()
    assert (alt[alt >= 0] % 2 == 1).all()
    nc = by["valid2_no_claimers"]
    got = nc.oracle()
    assert (got >= 0).sum() > 0 and not nc.info["claimers"][got[got >= 0]].any()
    assert (by["domino_200_head_masked"].oracle() == -1).all()


def test_oracle_equals_python_loop_on_every_class(classes):
    for name, cases in classes.items():
        for case in cases:
            v2 = np.ones(len(case.d2), np.uint8) if case.valid2 is None else case.valid2
            exp = py_brute_force(case.d1, case.a1, case.d2, case.a2, v2, case.ratio, case.check)
            assert np.array_equal(case.oracle(), exp), (name, case.name)
