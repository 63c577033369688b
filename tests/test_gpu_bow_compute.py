"""svgpu_bow_compute_batch on the device: every output compared as raw bits with (1) the loop of single transform calls followed by the
host accumulation and (2) the step-by-step restatement of tests/bow_compute_problems.py run on the restated descent.  Both forms; frame
sizes at the wave, workgroup and sort-path edges; empty frames; the order-sensitive one-word frame; the all-stop-word frame."""
import functools

import numpy as np
import pytest

from tests import bow_compute_problems as Q

pytestmark = pytest.mark.gpu
CASES = ("b1", "b2", "b33", "beyond_lds", "one_word")
FLAT = ("vec_off", "vec_word", "vec_weight", "feat_off", "feat_key", "feat_index")


@pytest.fixture(scope="module")
def ctx():
    from stella_vslam_amd.feature import Context
    return Context()


@functools.lru_cache(maxsize=None)
def _frames(form):
    from stella_vslam_amd import _lib
    return Q.frames(form, _lib.lib().svgpu_bow_compute_lds_capacity())


def _vocab(ctx, form, V):
    from stella_vslam_amd import data
    return data.bow_vocabulary(ctx, V["child_off"], V["children"], V["node_desc"], V["node_weight"], V["word_id"], V["depth"], framework=form, k=V["k"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, ref, what):
    for key in FLAT:
        assert got[key].dtype == ref[key].dtype and np.array_equal(_bits(got[key]), _bits(ref[key])), (what, key, got[key], ref[key])


def _single_calls(voc, form, sets):
    """the path that exists without the batch call: one transform call per frame, then the host accumulation"""
    parts = [(voc.descend_fbow(d, 2) if form == "fbow" else voc.descend(d, 2)) for d in sets]
    cat = lambda j, dt: np.concatenate([np.asarray(p[j]) for p in parts]).astype(dt)
    return cat(0, np.int32), cat(1, np.float32), cat(2, np.uint32)


@pytest.mark.parametrize("form", Q.FORMS)
@pytest.mark.parametrize("case", CASES)
def test_batch_equals_single_calls_and_restatement(ctx, form, case):
    p = _frames(form)[case]
    V, sets = p["vocab"], p["sets"]
    voc = _vocab(ctx, form, V)
    got = voc.compute_bow_batch(sets, levels_up=2)
    assert len(got["d_off"]) == len(sets) + 1
    word, weight, node = _single_calls(voc, form, sets)
    # the per-descriptor arrays equal the single calls on the same rows, and those the restated descent
    for key, ref in (("word", word), ("weight", weight), ("node", node)):
        assert np.array_equal(_bits(got[key]), _bits(ref)), (case, key)
    rw, rwt, rn = Q.descend(V, np.concatenate(sets), form, Q.level_of(V, form))
    assert np.array_equal(word, rw) and np.array_equal(_bits(weight), _bits(rwt)) and np.array_equal(node, rn)
    ref = Q.accumulate_batch(form, got["d_off"], word, weight, node)
    _same(got, ref, case)
    # what makes the case what it claims
    if case == "b33":
        assert (np.diff(got["vec_off"]) > 0).sum() >= 20 and (np.diff(got["vec_word"].astype(np.int64)) < 0).sum() >= 20  # ids ascend inside a frame only
        s = p["stop"]
        assert got["feat_off"][s + 1] - got["feat_off"][s] == (0 if form == "dbow2" else 40)
        assert (got["vec_off"][s + 1] == got["vec_off"][s]) == (form == "dbow2")
        d = p["distinct"]
        nv, nf = got["vec_off"][d + 1] - got["vec_off"][d], got["feat_off"][d + 1] - got["feat_off"][d]
        assert nv == nf >= 60 and (nf == 90 or form == "dbow2")  # every kept feature is a word of its own
    if case == "one_word":
        a, b = got["vec_off"][1], got["vec_off"][2]
        assert b - a == 1 and got["vec_word"][a] == Q.ONE_WORD
    if case == "beyond_lds":
        from stella_vslam_amd import _lib
        assert len(sets[1]) == _lib.lib().svgpu_bow_compute_lds_capacity() + 1
    voc.close()


@pytest.mark.parametrize("form", Q.FORMS)
def test_a_permutation_of_the_frames_permutes_the_results(ctx, form):
    p = _frames(form)["b33"]
    voc = _vocab(ctx, form, p["vocab"])
    base = voc.compute_bow_batch(p["sets"], levels_up=2)
    perm = np.random.default_rng(5).permutation(len(p["sets"]))
    got = voc.compute_bow_batch([p["sets"][i] for i in perm], levels_up=2)
    for j, i in enumerate(perm):
        for off, keys in (("vec_off", ("vec_word", "vec_weight")), ("feat_off", ("feat_key", "feat_index"))):
            for key in keys:
                a = got[key][got[off][j]:got[off][j + 1]]
                b = base[key][base[off][i]:base[off][i + 1]]
                assert np.array_equal(_bits(a), _bits(b)), (key, j, i)
    voc.close()


@pytest.mark.parametrize("form", Q.FORMS)
def test_launches_do_not_depend_on_the_number_of_frames(ctx, form):
    P = _frames(form)
    voc = _vocab(ctx, form, P["b1"]["vocab"])
    s1 = voc.compute_bow_batch(P["b1"]["sets"], levels_up=2)["stats"]
    s33 = voc.compute_bow_batch(P["b33"]["sets"], levels_up=2)["stats"]
    # descent, frame lookup, workgroup sort, run heads, two scans of one launch each (fewer than 16384 descriptors), emit, normalise;
    # one upload and one read-back; one synchronisation
    assert s1 == s33 == dict(launches=8, copies=2, synchronisations=1), (s1, s33)
    voc.close()


def _raw_call(ctx_, voc, which, good_off, good_desc, **over):
    """the C entry point on sentinel-filled outputs, `over` replacing single arguments of a good call -> (status, outputs)"""
    from stella_vslam_amd import _lib
    off, desc = good_off, good_desc
    n, b = int(off[-1]), len(off) - 1
    out = dict(word=np.full(n, -7, np.int32), weight=np.full(n, -7, np.float32), node=np.full(n, 7, np.uint32), vec_off=np.full(b + 1, -7, np.int32),
               vec_word=np.full(n, 7, np.uint32), vec_weight=np.full(n, -7.0), feat_off=np.full(b + 1, -7, np.int32), feat_key=np.full(n, 7, np.uint32),
               feat_index=np.full(n, -7, np.int32), stats=np.full(3, -7, np.int32))
    a = dict(ctx=ctx_.handle, vocab=voc._h, form=1 if which == "fbow" else 0, level=2, k=5, b=len(off) - 1, off=_lib.ptr(off), desc=_lib.ptr(desc),
             vec_off=_lib.ptr(out["vec_off"]), vec_word=_lib.ptr(out["vec_word"]), db=None, slots=None)
    a.update(over)
    rc = _lib.lib().svgpu_bow_compute_batch(a["ctx"], a["vocab"], a["form"], a["level"], a["k"], a["b"], a["off"], a["desc"], _lib.ptr(out["word"]),
                                           _lib.ptr(out["weight"]), _lib.ptr(out["node"]), a["vec_off"], a["vec_word"], _lib.ptr(out["vec_weight"]),
                                           _lib.ptr(out["feat_off"]), _lib.ptr(out["feat_key"]), _lib.ptr(out["feat_index"]), a["db"], a["slots"],
                                           _lib.ptr(out["stats"]))
    return rc, out


@pytest.mark.parametrize("form", Q.FORMS)
def test_bad_arguments_leave_every_output_untouched(ctx, form):
    from stella_vslam_amd import _lib, data
    p = _frames(form)["b2"]
    voc = _vocab(ctx, form, p["vocab"])
    desc = np.ascontiguousarray(np.concatenate(p["sets"]))
    off = np.array([0, 0, len(desc)], np.int32)
    rc, fresh = _raw_call(ctx, voc, form, off, desc)
    assert rc == 0 and fresh["vec_off"][0] == 0 and fresh["vec_off"][2] > 0  # the same call with good arguments writes
    db = data.bow_database(ctx, framework=form)
    bad = [dict(vocab=None), dict(off=None), dict(desc=None), dict(vec_off=None), dict(vec_word=None), dict(b=-1), dict(level=-1), dict(form=2),
           dict(off=_lib.ptr(np.array([0, 5, 3], np.int32))), dict(off=_lib.ptr(np.array([1, 1, 3], np.int32))), dict(db=db._h, slots=None)]
    if form == "fbow":
        bad += [dict(k=1), dict(k=1 << 20)]
    # (a vocabulary or database of another DEVICE is refused too; one device cannot show it)
    for over in bad:
        rc, out = _raw_call(ctx, voc, form, off, desc, **over)
        assert rc == 1, over
        for key, v in out.items():
            assert (v == (7 if v.dtype == np.uint32 else -7)).all(), (over, key)
    assert db.size() == (0, 0)
    db.close()
    voc.close()
