"""GPU parity of the CSR candidate matcher (k_cand_dist -> k_cand_replay_lds | k_cand_replay | k_area_replay) on its decision boundaries,
in every form the replay can take: every planted class of tests/cand_problems.py, embedded in padded tables that select the LDS-resident
form with 64, the two-chunk maximum, 5, 4, 3, 1 and 0 staged entries per list and the global-memory form (modes 0 - 3), and the LDS-state
and global-state forms of the AREA replay.  The form is asserted with svgpu_selftest_cand_replay_form -- the function the launch code
itself calls -- before every call; matches and count must equal O.match_candidates on the embedded problem, which is the padded answer
of the plain one."""
import numpy as np
import pytest

from tests import cand_problems as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd import feature
    return feature.Context()


@pytest.fixture(scope="module")
def forms():
    return P.find_forms()


def _gpu(ctx, c):
    from stella_vslam_amd import match
    if c.mode == P.AREA and c.thr == 50 and c.cand_skip is None and c.q_valid is None:  # what area::match_in_consistent_area can express
        return match.area(c.ratio, c.check, ctx).match_in_consistent_area(c.qdesc, c.q_angle, c.tdesc, c.t_angle, c.cand_off, c.cand_idx)
    return match.projection(c.ratio, c.check, ctx).match_candidates(c.qdesc, c.tdesc, c.cand_off, c.cand_idx, c.mode, c.thr, **c.kwargs())


def _run_class(ctx, forms, cls, form):
    nq, nt, want = forms[form]
    cases = [c for c in P.cases_of(cls) if form in P.forms_of(c.mode)]
    assert cases
    bad = []
    for c in cases:
        e, q_at, t_at = P.embed(c, nq, nt)
        assert P.replay_form(e.nq, e.nt, e.mode) == want == P.py_replay_form(e.nq, e.nt, e.mode), (c.name, form)
        exp = e.oracle()
        assert np.array_equal(exp, P.embedded_answer(c.oracle(), q_at, t_at, nq)), c.name
        got, num = _gpu(ctx, e)
        if not (np.array_equal(got, exp) and num == (exp >= 0).sum()):
            wrong = np.flatnonzero(got != exp)
            bad.append((c.name, form, [(int(np.searchsorted(q_at, q)), int(got[q]), int(exp[q])) for q in wrong[:6]], num, int((exp >= 0).sum())))
    assert not bad, bad  # (case, form, [(query of the plain case, got, expected)], num, expected num)


def _forms_for(cls):
    return [f for f in P.forms_of(P.RATIO) + P.forms_of(P.AREA) if any(f in P.forms_of(c.mode) for c in P.cases_of(cls))]


def _class_test(cls):
    @pytest.mark.parametrize("form", _forms_for(cls))
    def test(ctx, forms, form):
        _run_class(ctx, forms, cls, form)
    test.__name__ = test.__qualname__ = f"test_{cls}"
    test.__doc__ = P.CLASSES[cls].__doc__
    return test


test_threshold = _class_test("threshold")
test_ratio_equality = _class_test("ratio_equality")
test_same_octave = _class_test("same_octave")
test_triangulation_order = _class_test("triangulation_order")
test_ties = _class_test("ties")
test_gates = _class_test("gates")
test_head_exhaustion = _class_test("head_exhaustion")
test_claim_chains = _class_test("claim_chains")
test_area = _class_test("area")


def test_every_form_is_reached(forms):
    """the embeddings cover 64 staged entries, the two-chunk maximum, 5, 4, 3, 1, 0, the global form and both AREA forms"""
    assert sorted(v[2] for k, v in forms.items() if not k.startswith("area")) == sorted([64, forms["Kmax"][2], 5, 4, 3, 1, 0, -1])
    assert {forms["area_lds"][2], forms["area_global"][2]} == {0, 1}
    for cls in P.CLASSES:
        modes = {c.mode for c in P.cases_of(cls)}
        assert set(_forms_for(cls)) == {f for m in modes for f in P.forms_of(m)}
