"""The planted problems of tests/cand_problems.py do what they claim -- on the CPU, without the HIP library's kernels.

  * the literal restatement of the reference loops agrees with the oracle on every case of every class, plain and embedded in the padded
    tables that select each replay form;
  * every class drives the branch it is named after (planted distances hold, the designed answers are the oracle's, both verdicts occur,
    claim chains need the designed number of sweeps);
  * sensitivity: for every class, a deliberately wrong restatement differs from the oracle on at least one of its cases -- the evidence
    that tests/test_gpu_cand_edges.py would catch the corresponding kernel mistake;
  * svgpu_selftest_cand_replay_form (host only, the function the launch code itself calls) returns the form every embedding claims."""
import numpy as np
import pytest

from tests import cand_problems as P

CLASSES = list(P.CLASSES)


@pytest.fixture(scope="module")
def forms():
    from stella_vslam_amd import _lib
    _lib.build()
    return P.find_forms()


def _embedded(c, forms, name):
    nq, nt, _ = forms[name]
    e, q_at, t_at = P.embed(c, nq, nt)
    return e, q_at, t_at


@pytest.mark.parametrize("cls", CLASSES)
def test_restatement_equals_oracle(cls, forms):
    for c in P.cases_of(cls):
        exp = c.oracle()
        assert np.array_equal(P.py_match_candidates(c), exp), c.name
        names = P.forms_of(c.mode)
        for name in names:
            e, q_at, t_at = _embedded(c, forms, name)
            got = e.oracle()
            assert np.array_equal(got, P.embedded_answer(exp, q_at, t_at, e.nq)), (c.name, name)  # the expected answer is the padded original
            if name in (names[0], names[-1], "K1"):
                assert np.array_equal(P.py_match_candidates(e), got), (c.name, name)


@pytest.mark.parametrize("cls", CLASSES)
def test_class_drives_its_branch(cls):
    cases = P.cases_of(cls)
    accepted = rejected = 0
    for c in cases:
        assert np.array_equal(P.entry_distances(c), c.planted), c.name
        exp = c.oracle()
        designed = c.expect != -9
        assert np.array_equal(exp[designed], c.expect[designed]), (c.name, np.flatnonzero(designed & (exp != c.expect)))
        accepted += int((exp >= 0).sum())
        rejected += int((exp < 0).sum())
        assert c.nq <= 400 and c.nt <= 3000  # small enough for every form's tables
        if c.mode != P.AREA:
            fp, sweeps = P.py_fixed_point(c)
            assert np.array_equal(fp, exp), c.name
            if "chain" in c.info:
                assert sweeps >= c.info["chain"], (c.name, sweeps)
    assert accepted > 0 and rejected > 0
    n = {c.name: c for c in cases}
    lens = lambda c: np.diff(c.cand_off)
    if cls == "threshold":
        assert {(c.mode, c.thr) for c in cases} == {(m, t) for m in range(5) for t in (50, 100)}
        for c in cases:
            at_thr = [q for q in range(c.nq) if c.planted[c.cand_off[q]] == c.thr]
            assert len(at_thr) == 2 and all((c.oracle()[q] >= 0) == (c.mode != P.TRIANGULATION) for q in at_thr), c.name
    if cls == "ratio_equality":
        assert {c.mode for c in cases} == {P.RATIO_SAME_OCTAVE, P.RATIO, P.TRIANGULATION, P.AREA}
        assert np.float32(0.7) * np.float32(100) == np.float32(70) and 0.7 * 100 < 70 + 1e-9 and float(np.float32(0.7)) * 100 < 70
    if cls == "triangulation_order":
        assert sorted(set(lens(cases[0]).tolist())) == [3, 64, 65, 1025]
    if cls == "ties":
        for mode in ("best_only", "ratio"):
            assert lens(n[f"ties/positions/{mode}"]).tolist()[:6] == [b + 1 for _, b in P.TIE_POSITIONS]
    if cls == "gates":
        c = n["gates/ratio"]
        assert c.occupied.any() and c.cand_skip.any() and (c.t_xright == 0).any() and np.isnan(c.q_angle).any() and np.isnan(c.t_angle).any()
        assert ((c.t_xright > 0) & (c.t_xright < 1e-40)).any() and (lens(c) >= 65).sum() == 3
    if cls == "head_exhaustion":
        assert [c.info["K"] for c in cases] == list(P.SMALL_K)
        for c in cases:
            K = c.info["K"]
            assert {max(1, K - 1), K + 1, K + 5} <= set(lens(c).tolist()) | set((lens(c) - 2).tolist())
    if cls == "claim_chains":
        assert P.py_fixed_point(n["claim_chains/across_1024/ratio"])[1] == 40
    if cls == "area":
        c = n["area/take_over"]
        assert c.oracle()[0] == -1 and c.oracle()[2] >= 0  # the displaced holder is cleared
        assert (lens(n["area/second_on_another_lane"]) >= 65).all()


@pytest.mark.parametrize("cls,wrong", [(cls, w) for cls in CLASSES for w in P.SENSITIVITY[cls]])
def test_wrong_variant_is_caught(cls, wrong, forms):
    differs = []
    for c in P.cases_of(cls):
        e, _, _ = _embedded(c, forms, P.forms_of(c.mode)[1])  # two chunks of queries: chunk_blind needs the embedded indices
        if wrong == "head_stop":
            e_k, _, _ = _embedded(c, forms, f"K{c.info['K']}")
            assert forms[f"K{c.info['K']}"][2] == c.info["K"]
            if not np.array_equal(P.py_match_candidates(e_k, wrong, K=c.info["K"]), e_k.oracle()):
                differs.append(c.name)
            assert cls == "head_exhaustion" and differs and differs[-1] == c.name, c.name  # every K has to show it
        elif not np.array_equal(P.py_match_candidates(e, wrong), e.oracle()):
            differs.append(c.name)
    assert differs, f"no case of {cls} notices the mistake {wrong}"


def test_wrong_variants_cover_the_list():
    assert sorted(w for ws in P.SENSITIVITY.values() for w in ws) == sorted(P.WRONG)


def test_replay_form_export_and_restated_formula(forms):
    assert {k: v[2] for k, v in forms.items()} == {"K64": 64, "Kmax": forms["Kmax"][2], "K5": 5, "K4": 4, "K3": 3, "K1": 1, "K0": 0,
                                                     "global": -1, "area_lds": 1, "area_global": 0}
    for name, (nq, nt, want) in forms.items():
        mode = P.AREA if name.startswith("area") else P.RATIO
        assert P.replay_form(nq, nt, mode) == want == P.py_replay_form(nq, nt, mode), name
        if name not in ("K64",) and mode != P.AREA:
            assert nq > P.CHUNK  # two chunks of queries
    for mode in range(4):  # the form does not depend on the mode below AREA
        assert P.replay_form(1200, 21000, mode) == P.replay_form(1200, 21000, P.RATIO)
    rng = np.random.default_rng(5)
    for nq, nt in zip(rng.integers(0, 9000, 300).tolist(), rng.integers(0, 40000, 300).tolist()):
        for mode, wc in ((P.RATIO, 0), (P.RATIO, 1), (P.AREA, 0)):
            assert P.replay_form(nq, nt, mode, wc) == P.py_replay_form(nq, nt, mode, wc), (nq, nt, mode, wc)
    assert P.replay_form(-1, 5, 0) == -2 and P.replay_form(5, 5, 7) == -2
