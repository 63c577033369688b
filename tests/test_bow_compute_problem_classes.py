"""The problem classes of tests/bow_compute_problems.py exercise what they claim, and the step-by-step restatement of compute_bow agrees,
bit for bit, with the C++ host loop (tests/bow_compute_host_loop.cpp, the std::map loops of host/camera.cpp compiled alone).  No GPU."""
import functools
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from tests import bow_compute_problems as Q

ROOT = pathlib.Path(__file__).resolve().parent.parent


@functools.lru_cache(maxsize=None)
def _descents(form):
    """case -> (d_off, word, weight, node) of the restated descent"""
    out = {}
    for name, p in Q.frames(form).items():
        V, sets = p["vocab"], p["sets"]
        off = np.zeros(len(sets) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in sets])
        out[name] = (off, *Q.descend(V, np.concatenate(sets), form, Q.level_of(V, form)))
    return out


def _frame(form, case, f):
    off, word, weight, node = _descents(form)[case]
    return word[off[f]:off[f + 1]], weight[off[f]:off[f + 1]], node[off[f]:off[f + 1]]


@pytest.mark.parametrize("form", Q.FORMS)
def test_the_one_word_frame_is_order_sensitive(form):
    word, weight, node = _frame(form, "one_word", 1)
    assert len(word) == 300 and (word == Q.ONE_WORD).all() and (weight > 0).all()
    e = np.frexp(weight)[1]
    assert e.max() - e.min() >= 32  # the leaves hold exponents of -20 .. 20: about 40 binades, most of them reached
    s = Q.sum_in_order(weight)
    assert s != Q.sum_in_order(weight[::-1]) and s != Q.sum_pairwise(weight)
    vw, vv, _, _ = Q.accumulate(form, word, weight, node)
    assert list(vw) == [Q.ONE_WORD]
    # ... and so is the norm over the words of the frame behind it
    vw, vv, _, _ = Q.accumulate(form, *_frame(form, "one_word", 2))
    raw = {}
    w2, wt2, _ = _frame(form, "one_word", 2)
    for k, x in zip(w2, wt2):
        raw[int(k)] = raw.get(int(k), 0.0) + float(x)
    terms = [raw[k] * raw[k] if form == "fbow" else abs(raw[k]) for k in sorted(raw)]
    assert len(terms) >= 5
    n = Q.sum_in_order(terms)
    assert n != Q.sum_in_order(terms[::-1]) or n != Q.sum_pairwise(terms)


def test_the_stop_word_frame_yields_an_empty_vector():
    p = Q.frames("dbow2")["b33"]
    word, weight, node = _frame("dbow2", "b33", p["stop"])
    assert len(word) == 40 and (weight == 0).all()
    vw, vv, fk, fi = Q.accumulate("dbow2", word, weight, node)
    assert len(vw) == len(vv) == len(fk) == len(fi) == 0
    # the FBoW form keeps the words, with weight zero and no scaling
    word, weight, node = _frame("fbow", "b33", Q.frames("fbow")["b33"]["stop"])
    vw, vv, fk, fi = Q.accumulate("fbow", word, weight, node)
    assert len(vw) > 0 and (vv == 0).all() and len(fi) == 40


def test_the_fbow_class_has_a_leaf_above_the_store_level():
    p = Q.frames("fbow")["b33"]
    V = p["vocab"]
    leaf = V["child_off"][1:] == V["child_off"][:-1]
    store = Q.level_of(V, "fbow")
    above = set(np.flatnonzero(leaf & (V["level"] <= store)))  # found before the descent has made `store` steps
    assert above
    _, word, _, _ = _descents("fbow")["b33"]
    assert set(V["word_id"][list(above)]) & set(word.tolist())  # ... and descriptors of the class end there
    assert V["word_id"].max() == 2 ** 31 - 1 and (np.diff(np.sort(V["word_id"][leaf])) > 1).any() and (V["node_weight"][leaf] == 0).any()
    assert 3 <= np.diff(V["child_off"])[~leaf].min() and np.diff(V["child_off"]).max() <= 5


def test_sizes_reach_every_path():
    p = Q.frames("fbow")
    sizes = [len(s) for s in p["b33"]["sets"]]
    assert len(sizes) == 33 and sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1]
    assert {1, 63, 64, 65, 255, 256, 257} <= set(sizes)
    assert [len(s) for s in p["beyond_lds"]["sets"]] == [5, 4097, 66]
    word, _, _ = _frame("fbow", "b33", p["b33"]["distinct"])
    assert len(set(word.tolist())) == len(word) == 90


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/bow_compute_host_loop.cpp")
    exe = tmp_path_factory.mktemp("bowc") / "bow_compute_host_loop"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", str(ROOT / "tests" / "bow_compute_host_loop.cpp"),
                           "-o", str(exe)])
    return exe


@pytest.mark.parametrize("form", Q.FORMS)
@pytest.mark.parametrize("case", ("b33", "one_word", "beyond_lds"))
def test_restatement_equals_the_cpp_host_loop(host_loop, tmp_path, form, case):
    off, word, weight, node = _descents(form)[case]
    for f in range(len(off) - 1):
        w, wt, nd = word[off[f]:off[f + 1]], weight[off[f]:off[f + 1]], node[off[f]:off[f + 1]]
        src, dst = tmp_path / f"in{f}.bin", tmp_path / f"out{f}.bin"
        src.write_bytes(np.array([1 if form == "fbow" else 0, len(w)], np.int32).tobytes() + w.astype(np.int32).tobytes()
                        + wt.astype(np.float32).tobytes() + nd.astype(np.uint32).tobytes())
        r = subprocess.run([str(host_loop), str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0 and "bow compute host loop ok" in r.stdout, r.stdout + r.stderr
        raw = dst.read_bytes()
        nv, nf = np.frombuffer(raw, np.int32, 2)
        o = 8
        vw = np.frombuffer(raw, np.uint32, nv, o); o += 4 * nv
        vv = np.frombuffer(raw, np.uint64, nv, o); o += 8 * nv
        fk = np.frombuffer(raw, np.uint32, nf, o); o += 4 * nf
        fi = np.frombuffer(raw, np.int32, nf, o)
        ref = Q.accumulate(form, w, wt, nd)
        assert np.array_equal(vw, ref[0]) and np.array_equal(vv, ref[1].view(np.uint64)), (case, f)
        assert np.array_equal(fk, ref[2]) and np.array_equal(fi, ref[3]), (case, f)
