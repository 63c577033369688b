"""The keyframe BoW database restated on the CPU (data/bow_database.cc:58-159, data/bow_vocabulary.cc:9-16) as the literal sequential
loops, and the problem classes the CPU and GPU tests share.

A BoW vector is (ids, weights): ascending uint32 word ids, float64 weights.  A database is a list indexed by slot; None = erased.
Two score forms, as include/svgpu.h states them (both restated from the libraries' published sources: parity unpinned):
  "fbow"   fbow::BoWVector::score: weights rounded to float32, s += float64(v * w) with the product in float32,
           score = 1 if s >= 1 else 1 - sqrt(1 - s), returned as float32
  "dbow2"  DBoW2 L1Scoring::score: s += |v - w| - |v| - |w| in float64, score = -s / 2 as float32
"""
import math

import numpy as np

FORMS = ("fbow", "dbow2")


def vec(ids, weights):
    ids, weights = np.asarray(ids, np.uint32), np.asarray(weights, np.float64)
    assert len(ids) == len(weights) and (np.diff(ids.astype(np.int64)) > 0).all()
    return ids, weights


def as_dict(v):
    return {int(k): float(w) for k, w in zip(*v)}


def shared(q, k):
    """pairs (index in q, index in k) of the shared words in ascending word order: the merge both libraries' score loops perform"""
    (qi, _), (ki, _) = q, k
    out, a, b = [], 0, 0
    while a < len(qi) and b < len(ki):
        if qi[a] == ki[b]:
            out.append((a, b))
            a += 1
            b += 1
        elif qi[a] < ki[b]:
            a += 1
        else:
            b += 1
    return out


def raw_sum(form, q, k):
    """the ordered sum before the clamp / the halving (python floats are fp64; one rounding per operation)"""
    s = 0.0
    for a, b in shared(q, k):
        v, w = q[1][a], k[1][b]
        if form == "fbow":
            s += float(np.float32(v) * np.float32(w))
        else:
            v, w = float(v), float(w)
            s += math.fabs(v - w) - math.fabs(v) - math.fabs(w)
    return s


def finish(form, s):
    if form == "fbow":
        return np.float32(1.0 if s >= 1.0 else 1.0 - math.sqrt(1.0 - s))
    return np.float32(-s / 2.0)


def score(form, q, k):
    return finish(form, raw_sum(form, q, k))


def acquire(form, db, q, min_score=0.0, ratio=0.8, reject=()):
    """bow_database::acquire_keyframes -> dict(slots, common, score, max_common, thr, all_common); kept keyframes in ascending slot order"""
    rej = set(int(r) for r in reject)
    common = np.zeros(len(db), np.uint32)
    for slot, k in enumerate(db):
        if k is not None and slot not in rej:
            common[slot] = len(shared(q, k))
    mc = int(common.max(initial=0))
    empty = dict(slots=np.zeros(0, np.int32), common=np.zeros(0, np.uint32), score=np.zeros(0, np.float32), max_common=mc, thr=0, all_common=common)
    if mc == 0:
        return empty
    thr = int(np.float32(ratio) * np.float32(mc))  # a float product, truncated
    slots, cm, sc = [], [], []
    for slot in range(len(db)):
        if thr < common[slot]:
            f = score(form, q, db[slot])
            if np.float32(min_score) > f:
                continue
            slots.append(slot), cm.append(common[slot]), sc.append(f)
    return dict(empty, slots=np.array(slots, np.int32), common=np.array(cm, np.uint32), score=np.array(sc, np.float32), thr=thr)


def scores_of(form, db, q, slots):
    return np.array([-1.0 if not (0 <= s < len(db)) or db[s] is None else score(form, q, db[s]) for s in slots], np.float32)


# ------------------------------------------------------------------------------------------------ generators
def random_vec(rng, n, vocab, form, pool=None):
    ids = np.sort(rng.choice(vocab if pool is None else pool, n, replace=False)).astype(np.uint32)
    w = rng.uniform(0.05, 1.0, n)
    w = w / (np.sqrt((w * w).sum()) if form == "fbow" else np.abs(w).sum())
    return vec(ids, w)


def with_shared(rng, q, n_shared, n_other, vocab, form):
    """a vector sharing exactly n_shared words with q, plus n_other words q does not have"""
    other = np.setdiff1d(np.arange(vocab, dtype=np.uint32), q[0])
    ids = np.sort(np.concatenate([rng.choice(q[0], n_shared, replace=False), rng.choice(other, n_other, replace=False)])).astype(np.uint32)
    w = rng.uniform(0.05, 1.0, len(ids))
    w = w / (np.sqrt((w * w).sum()) if form == "fbow" else np.abs(w).sum())
    return vec(ids, w)


def Q(q, min_score=0.0, ratio=0.8, reject=()):
    return dict(q=q, min_score=float(min_score), ratio=float(ratio), reject=tuple(reject))


def problem_classes(form, stage=4096):
    """name -> dict(db, queries, vocab).  `stage`: the LDS staging capacity of the kernels (data.bowdb_query_stage_capacity())."""
    rng = np.random.default_rng(20261017)
    P = {}
    V = 600
    # ---- empty and tiny
    one = vec([7], [1.0])
    P["empty_database"] = dict(db=[], queries=[Q(one)], vocab=V)
    P["one_keyframe_one_word"] = dict(db=[one], queries=[Q(one), Q(vec([8], [1.0])), Q(vec([], []))], vocab=V)
    evens = [random_vec(rng, 30, V, form, pool=np.arange(0, V, 2)) for _ in range(5)]
    P["query_shares_nothing"] = dict(db=evens, queries=[Q(random_vec(rng, 40, V, form, pool=np.arange(1, V, 2)))], vocab=V)
    # ---- wave and chunk edges: keyframes of 1 .. 129 entries; queries of 1 entry and of one more than the staging capacity
    Vbig = stage * 3
    lens = [1, 63, 64, 65, 127, 128, 129]
    base = random_vec(rng, 129, Vbig, form)
    db = [vec(base[0][:n], base[1][:n]) for n in lens] + [random_vec(rng, n, Vbig, form) for n in lens]
    long_q = random_vec(rng, stage + 1, Vbig, form)
    # the last two words of the long query (the second one alone in its chunk) are shared with a keyframe that shares nothing else
    filler = np.setdiff1d(np.arange(long_q[0][-2], dtype=np.uint32), long_q[0])[:60]
    tail = vec(np.concatenate([filler, long_q[0][-2:]]), np.concatenate([rng.uniform(0.01, 0.2, len(filler)), [0.3, 0.4]]))
    db += [tail, vec(long_q[0][::7][:129], rng.uniform(0.01, 0.2, 129)), vec(long_q[0][-1:], [0.5])]
    P["wave_and_chunk_edges"] = dict(db=db, queries=[Q(vec(base[0][:1], base[1][:1]), ratio=0.0), Q(base, ratio=0.0), Q(base), Q(long_q, ratio=0.0), Q(long_q)],
                                     vocab=Vbig, stage=stage)
    # ---- the threshold: max_common = 7, ratio 0.8 -> thr = 5
    q = random_vec(rng, 10, V, form)
    db = [with_shared(rng, q, c, 20, V, form) for c in (5, 6, 7, 3, 0, 6)]
    P["threshold"] = dict(db=db, queries=[Q(q, ratio=0.8), Q(q, ratio=1.0), Q(q, ratio=0.0)], vocab=V)
    # ---- the score gate: min_score = the exact float32 score of one survivor, and the next float above it
    r = acquire(form, db, q, 0.0, 0.0)
    pick = float(np.sort(r["score"])[len(r["score"]) // 2])
    P["score_gate"] = dict(db=db, queries=[Q(q, min_score=pick, ratio=0.0), Q(q, min_score=float(np.nextafter(np.float32(pick), np.float32(2.0))), ratio=0.0)],
                           vocab=V, gate=pick)
    # ---- the clamp: a query identical to a stored vector; L2-normalised vectors whose restated sum lands on either side of 1
    hi = lo = None
    while hi is None or lo is None:
        v = random_vec(rng, int(rng.integers(20, 200)), V, "fbow")
        s = raw_sum("fbow", v, v)
        if s >= 1.0 and hi is None:
            hi = v
        if s < 1.0 and lo is None:
            lo = v
    P["clamp"] = dict(db=[hi, lo, random_vec(rng, 50, V, form)], queries=[Q(hi, ratio=0.0), Q(lo, ratio=0.0)], vocab=V)
    # ---- L1 terms: a shared word with equal weights (term -2|v|); vectors disjoint apart from a single word
    a = random_vec(rng, 40, V, form, pool=np.arange(0, 300))
    b = random_vec(rng, 40, V, form, pool=np.arange(300, 600))
    b = vec(np.concatenate([a[0][:1], b[0]]), np.concatenate([a[1][:1], b[1]]))
    P["l1_terms"] = dict(db=[a, b, vec(a[0], a[1][::-1].copy())], queries=[Q(a, ratio=0.0), Q(b, ratio=0.0)], vocab=V)
    # ---- reject list: rejecting the keyframe that holds max_common changes thr and so the result; rejecting everyone empties it
    q = random_vec(rng, 20, V, form)
    db = [with_shared(rng, q, c, 15, V, form) for c in (20, 12, 10, 16, 9)]
    P["reject"] = dict(db=db, queries=[Q(q), Q(q, reject=(0,)), Q(q, reject=(0, 1, 2, 3, 4)), Q(q, reject=(0, 99, -1))], vocab=V)
    # ---- cap overflow: five keyframes pass
    q = random_vec(rng, 12, V, form)
    P["five_pass"] = dict(db=[with_shared(rng, q, c, 10, V, form) for c in (10, 11, 1, 12, 10, 11, 0)], queries=[Q(q)], vocab=V)
    return P


def restate_class(form, p):
    return [acquire(form, p["db"], x["q"], x["min_score"], x["ratio"], x["reject"]) for x in p["queries"]]


def check_conditions(name, form, p, res):
    """what makes a pass on the class meaningful; asserted on the restatement by the CPU test (and again before the GPU comparison)"""
    if name == "empty_database":
        assert len(res[0]["slots"]) == 0 and res[0]["max_common"] == 0
    elif name == "one_keyframe_one_word":
        assert list(res[0]["slots"]) == [0] and res[0]["max_common"] == 1 and len(res[1]["slots"]) == 0 and len(res[2]["slots"]) == 0
    elif name == "query_shares_nothing":
        assert res[0]["max_common"] == 0 and len(res[0]["slots"]) == 0
    elif name == "wave_and_chunk_edges":
        assert [len(k[0]) for k in p["db"][:7]] == [1, 63, 64, 65, 127, 128, 129]
        assert list(res[1]["all_common"][:7]) == [1, 63, 64, 65, 127, 128, 129]          # every lane and chunk boundary counted
        assert len(p["queries"][0]["q"][0]) == 1 and res[0]["max_common"] == 1
        assert len(p["queries"][3]["q"][0]) == len(p["queries"][4]["q"][0]) == p["stage"] + 1  # one entry beyond the staging capacity
        assert res[3]["all_common"][14] == 2 and res[3]["all_common"][16] == 1          # words of the second chunk are found
        assert res[3]["all_common"][15] == 129 and 15 in res[4]["slots"] and len(res[3]["slots"]) > len(res[4]["slots"]) >= 1
    elif name == "threshold":
        r = res[0]
        assert r["max_common"] == 7 and r["thr"] == 5
        assert (r["all_common"] == r["thr"]).any() and (r["all_common"] == r["thr"] + 1).any()  # a keyframe exactly at thr, one just above
        assert list(r["slots"]) == [1, 2, 5]
        assert res[1]["thr"] == 7 and len(res[1]["slots"]) == 0
        assert res[2]["thr"] == 0 and list(res[2]["slots"]) == [0, 1, 2, 3, 5]
    elif name == "score_gate":
        g = np.float32(p["gate"])
        assert (res[0]["score"] == g).sum() >= 1 and not (res[1]["score"] == g).any()
        assert len(res[1]["slots"]) == len(res[0]["slots"]) - int((res[0]["score"] == g).sum()) and len(res[1]["slots"]) >= 1
    elif name == "clamp":
        s_hi, s_lo = raw_sum("fbow", p["db"][0], p["db"][0]), raw_sum("fbow", p["db"][1], p["db"][1])
        assert s_hi >= 1.0 > s_lo
        if form == "fbow":
            assert res[0]["score"][list(res[0]["slots"]).index(0)] == np.float32(1.0)
            assert res[1]["score"][list(res[1]["slots"]).index(1)] < np.float32(1.0)
    elif name == "l1_terms":
        a, b = p["db"][0], p["db"][1]
        assert len(shared(a, b)) == 1 and a[1][shared(a, b)[0][0]] == b[1][shared(a, b)[0][1]]  # one shared word, equal weights
        assert res[0]["all_common"][1] == 1 and res[0]["all_common"][2] == len(a[0])
        if form == "dbow2":
            assert raw_sum(form, a, b) == -2.0 * abs(float(a[1][shared(a, b)[0][0]]))
    elif name == "reject":
        assert res[0]["max_common"] == 20 and res[1]["max_common"] == 16
        assert list(res[0]["slots"]) != list(res[1]["slots"]) and len(res[1]["slots"]) > 0  # the rejection changes thr and the result
        assert not set(res[1]["slots"]) <= set(res[0]["slots"])
        assert len(res[2]["slots"]) == 0 and res[2]["max_common"] == 0
        assert list(res[3]["slots"]) == list(res[1]["slots"])
    elif name == "five_pass":
        assert list(res[0]["slots"]) == [0, 1, 3, 4, 5]
    else:
        raise KeyError(name)
