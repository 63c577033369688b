"""CPU: the sequential restatement of the keyframe BoW database (tests/bowdb_problems.py) against an independent second formulation --
dense vectors over the class's small vocabulary, np.intersect1d for the counts, math.fsum for the sums -- on every problem class, and
the conditions that keep a GPU pass on a class from being vacuous.

Counts, maxima, thresholds and the sets that pass the threshold are equal.  Scores agree within 4 float32 ulps: the two formulations add
the same terms in different orders (sequential against exactly rounded), which moves the fp64 sum by a few 1e-16 and the float32 score by
at most one rounding step; 4 leaves room for the sqrt of the FBoW form next to s = 1.  The min_score gate is compared with that same
allowance: a keyframe the restatement keeps has a dense score not more than 4 ulps below min_score, one it drops not more than 4 above."""
import math

import numpy as np
import pytest

from tests import bowdb_problems as B

STAGE = 4096  # SV_BOWDB_STAGE; test_binding_reports_the_staging_capacity_the_classes_are_built_for holds the two together


def dense(v, vocab):
    d, has = np.zeros(vocab, np.float64), np.zeros(vocab, bool)
    d[v[0]], has[v[0]] = v[1], True
    return d, has


def dense_score(form, q, k, vocab):
    (qd, qh), (kd, kh) = dense(q, vocab), dense(k, vocab)
    both = qh & kh
    if form == "fbow":
        terms = (qd.astype(np.float32) * kd.astype(np.float32))[both].astype(np.float64)
    else:
        terms = (np.abs(qd - kd) - np.abs(qd) - np.abs(kd))[both]
    return B.finish(form, math.fsum(terms.tolist()))


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.float32(max(abs(a), abs(b), np.float32(1e-30)))))


@pytest.fixture(scope="module", params=B.FORMS)
def classes(request):
    form = request.param
    P = B.problem_classes(form, STAGE)
    return form, P, {n: B.restate_class(form, p) for n, p in P.items()}


def test_class_conditions_hold(classes):
    form, P, R = classes
    assert len(P) >= 10
    for name, p in P.items():
        B.check_conditions(name, form, p, R[name])


def test_restatement_agrees_with_the_dense_formulation(classes):
    form, P, R = classes
    worst = 0.0
    for name, p in P.items():
        for x, r in zip(p["queries"], R[name]):
            rej = set(x["reject"])
            common = np.array([0 if k is None or s in rej else len(np.intersect1d(x["q"][0], k[0])) for s, k in enumerate(p["db"])], np.uint32)
            assert np.array_equal(common, r["all_common"]), name
            mc = int(common.max(initial=0))
            assert mc == r["max_common"], name
            if mc == 0:
                assert len(r["slots"]) == 0, name
                continue
            thr = int(np.float32(x["ratio"]) * np.float32(mc))
            assert thr == r["thr"], name
            passing = [s for s in range(len(p["db"])) if common[s] > thr]
            assert set(r["slots"]) <= set(passing), name
            ms = np.float32(x["min_score"])
            for s in passing:
                d = dense_score(form, x["q"], p["db"][s], p["vocab"])
                if s in set(r["slots"]):
                    f = r["score"][list(r["slots"]).index(s)]
                    worst = max(worst, ulps(d, f))
                    assert ulps(d, f) <= 4, (name, s, d, f)
                    assert d >= ms or ulps(d, ms) <= 4, (name, s, d, ms)
                    assert r["common"][list(r["slots"]).index(s)] == common[s]
                else:
                    assert d < ms or ulps(d, ms) <= 4, (name, s, d, ms)
    print(f"{form}: largest score deviation between the formulations {worst:.2f} float32 ulps")


def test_listed_slot_scores(classes):
    form, P, _ = classes
    p = P["threshold"]
    db = list(p["db"])
    db[2] = None
    q = p["queries"][0]["q"]
    got = B.scores_of(form, db, q, [0, 2, 4, 99, -1, 1])
    assert got[1] == got[3] == got[4] == -1.0
    assert got[2] == B.finish(form, 0.0)  # nothing shared: the empty sum
    for i, s in ((0, 0), (5, 1)):
        assert ulps(got[i], dense_score(form, q, db[s], p["vocab"])) <= 4


def test_binding_reports_the_staging_capacity_the_classes_are_built_for():
    """The GPU test builds its classes for data.bowdb_query_stage_capacity(); the classes checked here are built for the same number."""
    from stella_vslam_amd import _lib, data
    _lib.build()
    assert data.bowdb_query_stage_capacity() == STAGE
    assert hasattr(data, "bow_database")
