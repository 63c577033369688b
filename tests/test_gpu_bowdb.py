"""svgpu_bowdb_* on the device against the sequential CPU restatement of data::bow_database (tests/bowdb_problems.py): candidate slots and
shared-word counts equal, scores bit-equal as float32 -- the sum of a survivor is added in ascending word order on the device as in the
restatement, and the fp64 sqrt of the FBoW form is correctly rounded on both sides."""
import functools
import pathlib
import subprocess

import numpy as np
import pytest

from tests import bowdb_problems as B

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


@functools.lru_cache(maxsize=None)
def _classes(form):
    from stella_vslam_amd import data
    P = B.problem_classes(form, data.bowdb_query_stage_capacity())
    R = {n: B.restate_class(form, p) for n, p in P.items()}
    for n, p in P.items():
        B.check_conditions(n, form, p, R[n])
    return P, R


def _load(ctx, form, db):
    from stella_vslam_amd import data
    d = data.bow_database(ctx, framework=form)
    for i, v in enumerate(db):
        assert d.add_keyframe(v if v is not None else B.vec([1], [1.0])) == i
        if v is None:
            d.erase_keyframe(i)
    return d


def _same(got, ref, what):
    slots, common, score, n_out, mc = got
    assert mc == ref["max_common"], what
    assert n_out == len(ref["slots"]), (what, n_out, ref["slots"])
    assert np.array_equal(slots, ref["slots"]), (what, slots, ref["slots"])
    assert np.array_equal(common, ref["common"]), (what, common, ref["common"])
    assert np.array_equal(score.view(np.uint32), ref["score"].view(np.uint32)), (what, score, ref["score"])


def _acquire(d, x, **kw):
    return d.acquire_keyframes(x["q"], x["min_score"], x["ratio"], x["reject"], full=True, **kw)


CLASS_NAMES = ("empty_database", "one_keyframe_one_word", "query_shares_nothing", "wave_and_chunk_edges", "threshold", "score_gate", "clamp", "l1_terms",
               "reject", "five_pass")


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("name", CLASS_NAMES)
def test_candidates_and_scores_equal_the_restatement(ctx, form, name):
    P, R = _classes(form)
    assert set(P) == set(CLASS_NAMES)
    d = _load(ctx, form, P[name]["db"])
    for i, (x, r) in enumerate(zip(P[name]["queries"], R[name])):
        _same(_acquire(d, x), r, (name, i))
    d.close()


@pytest.mark.parametrize("form", B.FORMS)
def test_cap_overflow_writes_the_first_in_slot_order(ctx, form):
    P, R = _classes(form)
    p, r = P["five_pass"], R["five_pass"][0]
    d = _load(ctx, form, p["db"])
    slots, common, score, n_out, mc = _acquire(d, p["queries"][0], cap=2)
    assert n_out == 5 == len(r["slots"]) and mc == r["max_common"]
    assert np.array_equal(slots, r["slots"][:2]) and np.array_equal(common, r["common"][:2])
    assert np.array_equal(score.view(np.uint32), r["score"][:2].view(np.uint32))
    d.close()


@pytest.mark.parametrize("form", B.FORMS)
def test_batch_equals_single_calls(ctx, form):
    P, _ = _classes(form)
    p = P["wave_and_chunk_edges"]
    d = _load(ctx, form, p["db"])
    qs = [p["queries"][0]["q"], p["queries"][1]["q"], B.vec([], []), p["queries"][3]["q"], p["db"][9]]
    assert sorted(len(q[0]) for q in qs)[0] == 0 and max(len(q[0]) for q in qs) == p["stage"] + 1 and len(set(len(q[0]) for q in qs)) == 5
    ms = [0.0, 0.01, 0.0, 0.001, 0.5]
    batch = d.acquire_keyframes_batch(qs, ms, 0.3, reject=(3,))
    kept = 0
    for q, m, b in zip(qs, ms, batch):
        s = d.acquire_keyframes(q, m, 0.3, (3,), full=True)
        for x, y in zip(s[:3], b[:3]):
            assert x.tobytes() == y.tobytes()
        assert s[3:] == b[3:]
        _same(b, B.acquire(form, p["db"], q, m, 0.3, (3,)), len(q[0]))
        kept += b[3]
    assert kept >= 4 and batch[2][3] == 0
    d.close()


@pytest.mark.parametrize("form", B.FORMS)
def test_scores_of_listed_slots(ctx, form):
    P, _ = _classes(form)
    p = P["threshold"]
    db = list(p["db"])
    d = _load(ctx, form, db)
    q = p["queries"][0]["q"]
    kept = d.acquire_keyframes(q, 0.0, 0.0)
    d.erase_keyframe(2)
    db[2] = None
    listed = [0, 2, 4, 99, -1, 1, 5, 3]
    got = d.score(q, listed)
    ref = B.scores_of(form, db, q, listed)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (got, ref)
    assert got[1] == got[3] == got[4] == -1.0
    for s, f in zip(kept[0], kept[2]):  # the survivors' scores of acquire are the listed ones
        if s != 2:
            assert got[listed.index(int(s))] == f
    d.close()


@pytest.mark.parametrize("form", B.FORMS)
def test_mutation_growth_compaction_clear(ctx, form):
    rng = np.random.default_rng(5)
    V = 2000
    q = B.random_vec(rng, 150, V, form)
    mk = lambda: B.with_shared(rng, q, int(rng.integers(5, 140)), int(rng.integers(1, 30)), V, form)
    db = [mk() for _ in range(20)]
    d = _load(ctx, form, db)
    cap0 = d.diagnostics()["pool_capacity"]
    best = int(np.argmax(B.acquire(form, db, q, 0.0, 0.0)["all_common"]))
    d.erase_keyframe(best)
    db[best] = None
    r = B.acquire(form, db, q)
    assert best not in r["slots"] and len(r["slots"]) >= 1
    _same(d.acquire_keyframes(q, full=True), r, "after erasing the best")
    for _ in range(40):  # beyond the initial pool: one growth
        db.append(mk())
        assert d.add_keyframe(db[-1]) == len(db) - 1
    g = d.diagnostics()
    assert g["num_growths"] >= 1 and g["pool_capacity"] > cap0 and g["num_compactions"] == 0 and g["pool_used"] > cap0
    for s in range(0, 45):  # more than half of the pool dead: a compaction
        d.erase_keyframe(s)
        db[s] = None
    g2 = d.diagnostics()
    assert g2["num_compactions"] >= 1 and g2["pool_used"] < g["pool_used"] // 2 + 200 and g2["num_slots"] == 60
    live = [k for k in db if k is not None]
    assert d.size() == (len(live), sum(len(k[0]) for k in live))
    for ratio in (0.8, 0.0):
        _same(d.acquire_keyframes(q, 0.0, ratio, full=True), B.acquire(form, db, q, 0.0, ratio), ("after compaction", ratio))
    before = (d.size(), d.diagnostics())
    d.erase_keyframe(3), d.erase_keyframe(3), d.erase_keyframe(1000), d.erase_keyframe(-5)  # erased twice, unknown: no-ops
    assert (d.size(), d.diagnostics()) == before
    d.clear()
    assert d.size() == (0, 0) and d.acquire_keyframes(q, full=True)[3:] == (0, 0)
    db = [mk() for _ in range(3)]
    for i, v in enumerate(db):
        assert d.add_keyframe(v) == i  # slot numbers start again
    _same(d.acquire_keyframes(q, 0.0, 0.0, full=True), B.acquire(form, db, q, 0.0, 0.0), "after clear")
    d.close()


def test_unsorted_vector_is_refused(ctx):
    from stella_vslam_amd import data
    from stella_vslam_amd._lib import SvgpuError
    d = data.bow_database(ctx)
    for ids in ([3, 2], [4, 4]):
        with pytest.raises(SvgpuError) as e:
            d.add_keyframe((np.array(ids, np.uint32), np.ones(2)))
        assert e.value.status == 1
    assert d.size() == (0, 0)
    d.close()


# ------------------------------------------------------------------------------------------------ vectors of a vocabulary
@functools.lru_cache(maxsize=None)
def _map(form):
    """300 keyframes of synthetic descriptors through bow_vocabulary.transform; every 25th is a near-duplicate of the query's keyframe"""
    from stella_vslam_amd import data
    from stella_vslam_amd.feature import Context
    from tests.test_oracle_bow import make_tree
    ctx = Context()
    rng = np.random.default_rng(11)
    tree = make_tree(rng, k=10, depth=3)
    voc = data.bow_vocabulary(ctx, tree["child_off"], tree["children"], tree["node_desc"], tree["node_weight"], tree["word_id"], tree["depth"], framework=form)
    leaves = np.flatnonzero(tree["word_id"] >= 0)

    def descriptors(n):
        d = tree["node_desc"][rng.choice(leaves, n)].copy()
        for r in d:
            for b in rng.integers(0, 256, 3):
                r[b // 8] ^= 1 << (b % 8)
        return d

    qd = descriptors(150)
    descs = []
    for i in range(300):
        if i % 25 == 7:
            d = qd.copy()
            d[rng.choice(150, 15, replace=False)] = descriptors(15)
        else:
            d = descriptors(150)
        descs.append(d)
    vecs = [voc.transform(d)[0] for d in descs]
    to_vec = lambda bv: B.vec(list(bv.keys()), list(bv.values()))
    return dict(ctx=ctx, voc=voc, qd=qd, q=voc.transform(qd)[0], descs=descs, dicts=vecs, db=[to_vec(v) for v in vecs], to_vec=to_vec)


@pytest.mark.parametrize("form", B.FORMS)
def test_vocabulary_vectors_with_near_duplicates(form):
    from stella_vslam_amd import data
    m = _map(form)
    d = data.bow_database(m["ctx"], framework=form)
    for i, bv in enumerate(m["dicts"]):  # the dicts bow_vocabulary.transform returns go in as they are
        assert d.add_keyframe(bv) == i
    q = m["to_vec"](m["q"])
    for ratio, min_score in ((0.8, 0.0), (0.3, 0.05), (0.0, 0.0)):
        r = B.acquire(form, m["db"], q, min_score, ratio)
        if ratio > 0:
            assert 0 < len(r["slots"]) < 300 and set(range(7, 300, 25)) <= set(r["slots"])  # neither empty nor everything
        _same(d.acquire_keyframes(m["q"], min_score, ratio, full=True), r, ratio)
    d.close()


def test_candidates_feed_the_bow_matcher():
    """The candidates of a query keyframe go to svgpu_bow_match through the existing binding: the near-duplicate gives more matches than
    the survivor with the lowest score."""
    from stella_vslam_amd import data, match
    m = _map("dbow2")
    d = data.bow_database(m["ctx"], framework="dbow2")
    for bv in m["dicts"]:
        d.add_keyframe(bv)
    slots, common, score = d.acquire_keyframes(m["q"], 0.0, 0.0)
    assert len(slots) > 20
    dup, other = int(slots[np.argmax(score)]), int(slots[np.argmin(score)])
    assert dup % 25 == 7 and other % 25 != 7
    bt = match.bow_tree(0.8, False, m["ctx"])
    node_q = m["voc"].descend(m["qd"])[2]
    ones, zeros = np.ones(150, np.uint8), np.zeros(150, np.float32)
    n = {}
    for s in (dup, other):
        n[s] = bt.match_keyframes(m["qd"], zeros, ones, node_q, m["descs"][s], zeros, m["voc"].descend(m["descs"][s])[2])[1]
    assert n[dup] >= 100 and n[dup] > n[other], n
    d.close()


def test_drop_in_class_against_the_map_and_list_transcription():
    """host/drop_in/bow_database_hip on stand-in keyframes: candidate sets equal those of a host transcription of the reference's
    inverted-index algorithm, for both score forms."""
    exe = ROOT / "stella_vslam_amd" / "host" / "test_bow_database"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bow_database ok" in out.stdout
