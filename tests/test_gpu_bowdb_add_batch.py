"""svgpu_bowdb_add_batch and the registration path of svgpu_bow_compute_batch against B single svgpu_bowdb_add calls on a second database:
slots, size and diagnostics, and every later acquire / acquire_batch / score as raw bits -- after a plain batch, after erasing a third of
the slots past the compaction threshold, and after a pool growth the batch itself forces."""
import functools

import numpy as np
import pytest

from tests import bow_compute_problems as Q

pytestmark = pytest.mark.gpu
POOL_INITIAL = 4096  # entries of a database's first pools (svgpu_bowdb.hip)


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


@functools.lru_cache(maxsize=None)
def _rounds(form):
    """three rounds of descriptor sets: every third frame of round 0 long (erasing those passes the compaction threshold), an empty frame
    in round 1, and a round 2 whose vectors alone outgrow the first pools"""
    rng = np.random.default_rng(77)
    V = Q.toy_vocabulary(7, 4)
    mk = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return V, [[mk(300 if i % 3 == 0 else 12) for i in range(18)], [mk(n) for n in (40, 0, 65, 7, 130)], [mk(400) for _ in range(40)]]


def _vocab(ctx, form, V):
    from stella_vslam_amd import data
    return data.bow_vocabulary(ctx, V["child_off"], V["children"], V["node_desc"], V["node_weight"], V["word_id"], V["depth"], framework=form, k=V["k"])


def _state(db, queries):
    """everything a later caller can see of the database, floats as bits"""
    d = db.diagnostics()
    slots = np.arange(-1, d["num_slots"] + 1, dtype=np.int32)
    out = [db.size(), {k: d[k] for k in ("num_slots", "pool_capacity", "pool_used", "num_compactions")}]
    for q in queries:
        s, c, sc, n, mc = db.acquire_keyframes(q, 0.0, 0.3, full=True)
        out.append((s.tolist(), c.tolist(), sc.view(np.uint32).tolist(), n, mc, db.score(q, slots).view(np.uint32).tolist()))
    for s, c, sc, n, mc in db.acquire_keyframes_batch(queries, 0.0, 0.3, reject=(1,)):
        out.append((s.tolist(), c.tolist(), sc.view(np.uint32).tolist(), n, mc))
    return out


@pytest.mark.parametrize("form", Q.FORMS)
@pytest.mark.parametrize("path", ("add_batch", "fused"))
def test_database_equals_single_adds(ctx, form, path):
    from stella_vslam_amd import data
    V, rounds = _rounds(form)
    voc = _vocab(ctx, form, V)
    got, ref = data.bow_database(ctx, framework=form), data.bow_database(ctx, framework=form)
    queries = None
    for r, sets in enumerate(rounds):
        vecs = [v for v, _ in voc.transform_batch(sets, levels_up=2)]
        if queries is None:
            queries = [vecs[0], vecs[4], vecs[7], {}]
        before = got.diagnostics()
        if path == "add_batch":
            slots = got.add_keyframes(vecs)
        else:
            res, slots = voc.transform_batch(sets, levels_up=2, db=got)
            assert [v for v, _ in res] == vecs
        first = ref.diagnostics()["num_slots"]
        assert slots == [ref.add_keyframe(v) for v in vecs] == list(range(first, first + len(vecs)))  # handed out in order
        assert _state(got, queries) == _state(ref, queries), (path, r)
        if r == 0:  # the long frames hold more than half of the pool: the erases end in a compaction
            for s in range(0, len(vecs), 3):
                got.erase_keyframe(s), ref.erase_keyframe(s)
            assert got.diagnostics()["num_compactions"] == ref.diagnostics()["num_compactions"] >= 1
            assert _state(got, queries) == _state(ref, queries)
        if r == 2:  # this batch alone did not fit: one growth check made room for all of it
            total = sum(len(v) for v in vecs)
            assert total > POOL_INITIAL and before["pool_used"] + total > before["pool_capacity"]
            assert got.diagnostics()["pool_capacity"] > before["pool_capacity"] and got.diagnostics()["num_growths"] == before["num_growths"] + 1
    got.close(), ref.close(), voc.close()


@pytest.mark.parametrize("form", Q.FORMS)
def test_a_batch_with_one_descending_frame_is_rejected_whole(ctx, form):
    from stella_vslam_amd import _lib, data
    V, rounds = _rounds(form)
    voc = _vocab(ctx, form, V)
    vecs = [v for v, _ in voc.transform_batch(rounds[1], levels_up=2)]
    db = data.bow_database(ctx, framework=form)
    assert db.add_keyframes(vecs[:2]) == [0, 1]
    queries = [vecs[0], vecs[2]]
    before = _state(db, queries)
    arrs = [data._bow_arrays(v) for v in vecs]
    w3 = arrs[2][0].copy()
    w3[[1, 2]] = w3[[2, 1]]  # the third frame's ids no longer ascend
    off = np.zeros(len(arrs) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a, _ in arrs])
    words = np.concatenate([a if i != 2 else w3 for i, (a, _) in enumerate(arrs)]).astype(np.uint32)
    weights = np.concatenate([b for _, b in arrs])
    slots = np.full(len(arrs), -7, np.int32)
    rc = _lib.lib().svgpu_bowdb_add_batch(ctx.handle, db._h, len(arrs), _lib.ptr(off), _lib.ptr(words), _lib.ptr(weights), _lib.ptr(slots))
    assert rc == 1 and (slots == -7).all()
    assert _state(db, queries) == before
    with pytest.raises(Exception):
        db.add_keyframes([vecs[0], (w3, arrs[2][1])])
    assert _state(db, queries) == before
    db.close(), voc.close()


@pytest.mark.parametrize("form", Q.FORMS)
def test_registration_issues_the_same_work_for_one_frame_and_for_33(ctx, form):
    """no growth in either call (the first pools hold 4096 entries and 256 slots): the workgroup-path launches of the call without a
    database; one upload, the offsets' read-back, one copy per pool, the slot records, one read-back of the results; two synchronisations"""
    from stella_vslam_amd import data
    P = Q.frames(form)
    voc = _vocab(ctx, form, P["b1"]["vocab"])
    db = data.bow_database(ctx, framework=form)
    r1 = voc.compute_bow_batch(P["b1"]["sets"], levels_up=2, db=db)
    r33 = voc.compute_bow_batch(P["b33"]["sets"], levels_up=2, db=db)
    d = db.diagnostics()
    assert d["num_growths"] == 0 and d["num_slots"] == 34 and d["pool_used"] == r1["vec_off"][-1] + r33["vec_off"][-1] <= POOL_INITIAL
    assert list(r1["slots"]) == [0] and list(r33["slots"]) == list(range(1, 34))
    assert r1["stats"] == r33["stats"] == dict(launches=8, copies=6, synchronisations=2), (r1["stats"], r33["stats"])
    db.close(), voc.close()
