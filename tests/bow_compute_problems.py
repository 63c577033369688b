"""compute_bow restated on the CPU, step by step (data/bow_vocabulary.cc:18-24 as stella_vslam_amd/host/camera.cpp
bow_vocabulary_hip::compute_bow spells it out), and the toy vocabularies and frames the CPU and GPU tests of svgpu_bow_compute_batch share.

Two forms, as include/svgpu.h states them:
  "fbow"   every feature takes part; word weight = 0.0 + w[i0] + w[i1] + ... in ascending feature index (fp64 adds of the fp32 weights);
           norm = sum over the words in ascending id of v * v (product rounded, then added); if norm > 0: v *= 1.0 / sqrt(norm)
  "dbow2"  only features with weight > 0; the same word sums; norm = sum of fabs(v); if norm > 0: v /= norm
Python floats are fp64 and every operation below rounds once: the loops are the arithmetic, not an approximation of it.
"""
import math

import numpy as np

FORMS = ("fbow", "dbow2")
ONE_WORD = 123456789
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


# ------------------------------------------------------------------------------------------------ vocabularies
def toy_vocabulary(seed, depth, one_word=False):
    """A random tree: branching 3 to 5, leaves down to `depth` and some above it (from depth 1 on), word ids not contiguous and up to
    2**31 - 1, about one leaf in six with weight zero.  one_word=True: every other leaf carries the SAME word id ONE_WORD and a weight
    of their own, spread over about 40 binades -- the only way features of one word differ in weight."""
    rng = np.random.default_rng(seed)
    kids, level = [[]], [0]
    frontier = [0]
    for d in range(1, depth + 1):
        nxt = []
        for parent in frontier:
            for _ in range(int(rng.integers(3, 6))):
                node = len(kids)
                kids.append([])
                level.append(d)
                kids[parent].append(node)
                if d < depth and rng.random() > 0.2:  # one in five stops early: a leaf above the deepest level
                    nxt.append(node)
        frontier = nxt
    n = len(kids)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(k) for k in kids])
    leaves = [i for i in range(n) if not kids[i]]
    word, weight = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    if one_word:
        shared = rng.random(len(leaves)) < 0.5  # the other leaves are words of their own: a frame's norm has several terms
        word[leaves] = np.where(shared, ONE_WORD, 1000 + 37 * np.arange(len(leaves))).astype(np.int32)
        weight[leaves] = (rng.uniform(1.0, 2.0, len(leaves)) * np.exp2(rng.integers(-20, 21, len(leaves)))).astype(np.float32)
    else:
        ids = np.sort(rng.choice(2 ** 31 - 2, len(leaves) - 1, replace=False))
        ids = np.concatenate([ids, [2 ** 31 - 1]])
        word[leaves] = rng.permutation(ids).astype(np.int32)
        w = rng.uniform(0.01, 4.0, len(leaves)).astype(np.float32)
        w[rng.random(len(leaves)) < 1 / 6] = 0.0
        weight[leaves] = w
    return dict(child_off=off, children=np.array([c for k in kids for c in k], np.int32), node_desc=rng.integers(0, 256, (n, 32), dtype=np.uint8),
                node_weight=weight, word_id=word, depth=depth, k=5, level=np.array(level, np.int32))


def descend(V, desc, form, level):
    """k_bow_descend / k_fbow_descend restated per descriptor -> (word int32, weight float32, node uint32)"""
    off, ch, nd = V["child_off"], V["children"], V["node_desc"]
    nbits = 0
    while (1 << nbits) < V["k"]:
        nbits += 1
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    word, weight, node = np.zeros(len(desc), np.int32), np.zeros(len(desc), np.float32), np.zeros(len(desc), np.uint32)
    for f, d in enumerate(desc):
        cur, lev, nid, code, key = 0, 0, 0, 0, 0
        beg, end = int(off[0]), int(off[1])
        while end > beg:
            dist = _POP[nd[ch[beg:end]] ^ d].sum(axis=1)
            best = beg + int(np.argmin(dist))  # the first child keeps ties
            child = int(ch[best])
            if form == "fbow":
                if lev == level:
                    key = code
                cur = child
                if off[child + 1] == off[child]:
                    if lev < level:
                        key = code
                    break
                code = ((code << nbits) | (best - beg)) & 0xFFFFFFFF
                lev += 1
            else:
                lev += 1
                cur = child
                if lev == level:
                    nid = cur
            beg, end = int(off[child]), int(off[child + 1])
        word[f], weight[f], node[f] = V["word_id"][cur], V["node_weight"][cur], key if form == "fbow" else nid
    return word, weight, node


def level_of(V, form, levels_up=2):
    return levels_up if form == "fbow" else max(V["depth"] - levels_up, 0)


# ------------------------------------------------------------------------------------------------ the arithmetic
def accumulate(form, word, weight, node):
    """one frame's compute_bow from its descent arrays -> (vec_word uint32, vec_weight float64, feat_key uint32, feat_index int32)"""
    bow, feat = {}, {}
    for i in range(len(word)):
        w = float(weight[i])  # (double)weight[i]
        if form == "dbow2" and not (w > 0.0):
            continue
        key = int(word[i]) & 0xFFFFFFFF
        bow[key] = bow.get(key, 0.0) + w
        feat.setdefault(int(node[i]) & 0xFFFFFFFF, []).append(i)
    words = sorted(bow)
    norm = 0.0
    for k in words:
        v = bow[k]
        norm += v * v if form == "fbow" else math.fabs(v)
    if norm > 0.0:
        if form == "fbow":
            r = 1.0 / math.sqrt(norm)
            for k in words:
                bow[k] = bow[k] * r
        else:
            for k in words:
                bow[k] = bow[k] / norm
    fk = [k for k in sorted(feat) for _ in feat[k]]
    fi = [i for k in sorted(feat) for i in feat[k]]
    return (np.array(words, np.uint32), np.array([bow[k] for k in words], np.float64), np.array(fk, np.uint32), np.array(fi, np.int32))


def accumulate_batch(form, d_off, word, weight, node):
    """every frame's accumulate(), flattened as svgpu_bow_compute_batch returns it"""
    parts = [accumulate(form, word[a:b], weight[a:b], node[a:b]) for a, b in zip(d_off[:-1], d_off[1:])]
    cat = lambda j, dt: np.concatenate([p[j] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    vec_off, feat_off = np.zeros(len(parts) + 1, np.int32), np.zeros(len(parts) + 1, np.int32)
    vec_off[1:] = np.cumsum([len(p[0]) for p in parts])
    feat_off[1:] = np.cumsum([len(p[2]) for p in parts])
    return dict(vec_off=vec_off, vec_word=cat(0, np.uint32), vec_weight=cat(1, np.float64), feat_off=feat_off, feat_key=cat(2, np.uint32),
                feat_index=cat(3, np.int32))


def sum_in_order(values):
    s = 0.0
    for v in values:
        s += float(v)
    return s


def sum_pairwise(values):
    v = [float(x) for x in values]
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else 0.0


# ------------------------------------------------------------------------------------------------ frames
def _pool(V, form, rng, n):
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return desc, descend(V, desc, form, level_of(V, form))


def frames(form, lds_cap=4096):
    """name -> dict(vocab, sets): the descriptor sets of one svgpu_bow_compute_batch call each.  Sizes are the smallest at which the
    kernels can go wrong: wave and workgroup edges (63 .. 257), frame boundaries inside a wave, empty frames first / in the middle / last,
    and one frame one descriptor beyond the workgroup path between two small ones."""
    rng = np.random.default_rng(20261021)
    V = toy_vocabulary(7, 4)
    pool, (pw, pwt, _) = _pool(V, form, rng, 6000)
    take = lambda n: pool[rng.choice(len(pool), n, replace=False)]
    P = {}
    P["b1"] = dict(vocab=V, sets=[take(65)])
    P["b2"] = dict(vocab=V, sets=[take(0), take(257)])
    # all stop words (DBoW2: an empty vector, no division); all words distinct
    stop = pool[pwt == 0][:40]
    _, first = np.unique(pw, return_index=True)
    distinct = pool[np.sort(first)][:90]
    sizes = [0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 3, 5, 7, 11, 13, 2, 17, 0, 29, 31, 33, 1, 1, 1, 40, 23, 19, 9]
    sets = [take(n) for n in sizes] + [stop, distinct, take(6), take(128), take(0)]
    assert len(sets) == 33
    P["b33"] = dict(vocab=V, sets=sets, stop=len(sizes), distinct=len(sizes) + 1)
    P["beyond_lds"] = dict(vocab=V, sets=[take(5), pool[rng.choice(len(pool), lds_cap + 1, replace=True)], take(66)])
    # 300 descriptors in ONE word whose features differ in weight over ~40 binades; behind it a frame of many words of such weights
    W = toy_vocabulary(11, 3, one_word=True)
    wpool, (ww, _, _) = _pool(W, form, rng, 1200)
    P["one_word"] = dict(vocab=W, sets=[take(4), wpool[ww == ONE_WORD][:300], wpool[:150]])
    assert len(P["one_word"]["sets"][1]) == 300
    return P
