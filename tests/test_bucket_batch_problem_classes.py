"""The batches of tests/bucket_batch_problems.py are what they claim (by the CPU oracle), the designed answers of the planted classes
are the oracle's, a literal restatement of the batched logic agrees with the oracle on every class while two deliberately wrong variants
of it do not (so the classes can catch those faults), and the C header carries the additions.  No GPU."""
import pathlib
import re

import numpy as np
import pytest

from tests import bucket_batch_problems as BP
from tests.host_check import build_and_run

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", BP.CLASSES)
def test_classes_are_what_they_claim(name):
    b = BP.batch(name)
    for ori in (True, False):
        ref = BP.oracle(b, ori)
        if not name.startswith("planted"):
            for p, (m, n) in enumerate(ref):
                assert (n == 0) == (p in b["degenerate"]), (name, p, n)
                assert n == int((m >= 0).sum())
        if "expect" in b:
            ex = b["expect"](ori)
            assert sum(e is not None for e in ex) >= len(ex) - 1
            for p, e in enumerate(ex):
                assert e is None or np.array_equal(e, ref[p][0]), (name, ori, p)


def test_shapes():
    r = BP.batch("reloc")
    assert isinstance(r["side2"], dict) and len(r["side1"]) == 6 and r["side1"][1] is r["side1"][2]
    assert not r["side1"][3]["valid"].any() and len(r["side1"][4]["desc"]) == 0 and r["side2"]["occupied"].any()
    assert not np.intersect1d(r["side1"][5]["node"], r["side2"]["node"]).size
    lp = BP.batch("loop")
    assert isinstance(lp["side1"], dict) and [len(s["desc"]) for s in lp["side2"]][-1] == 1 and len({len(s["desc"]) for s in lp["side2"]}) == 5
    assert [len(s["desc"]) for s in BP.batch("unshared")["side1"]] == [1, 64, 700]
    for name in ("tri_bow", "tri_robust"):
        t = BP.batch(name)
        assert isinstance(t["side1"], dict) and len(t["side2"]) == 4 and set(t["valid_epipole"]) == {0, 1}
        assert (t["side1"]["node"] is None) == (name == "tri_robust") and not np.array_equal(t["E_12"][0], t["E_12"][2])
    p = BP.batch("planted_eq")
    buckets = {int((s["node"] == 0).sum()) for s in p["side2"]}
    assert set(BP.REGIME_BUCKETS) <= buckets and max(len(s["desc"]) for s in p["side1"]) == BP.CHAIN > 1024
    assert {BP.batch(n)["lowe_ratio"] for n in ("planted_lo", "planted_eq", "planted_hi")} == {float(np.nextafter(np.float32(0.75), np.float32(0))), 0.75,
                                                                                                float(np.nextafter(np.float32(0.75), np.float32(1)))}
    s = BP.batch("spill")
    n = BP.SPILL_N
    assert [len(x["desc"]) for x in s["side1"]] == [64, n, 64]
    assert (3 * n + 1) * 4 + 3 * ((n + 3) & ~3) + 16 > 150 * 1024  # cand_lds_bytes(n, n, 0) of match_kernels.hip: beyond the budget, the global-memory replay
    assert BP.num_problems(BP.batch("many")) == 300
    # sides on both sides of the one-workgroup sort's limit (the radix fallback beyond it), and n1 beyond the short scan in every single call
    lim = BP.SORT_SMALL_MAX
    assert f"#define SV_SORT_SMALL_MAX {lim}" in (ROOT / "stella_vslam_amd" / "csrc" / "sv_sort.h").read_text()
    ls = BP.batch("long_sides")
    assert ls["kind"] == "bow" and isinstance(ls["side1"], dict) and len(ls["side1"]["desc"]) == 20000 > lim
    assert [len(x["desc"]) for x in ls["side2"]] == [lim + 1, 300, lim, 0]
    assert all(len(BP.sides(ls, p)[0]["desc"]) > lim for p in range(BP.num_problems(ls)))  # sv_bucket_count's long scan
    for x in [ls["side1"]] + ls["side2"][:3]:
        node = np.asarray(x["node"])
        assert (node < 0).any() and np.bincount(np.unique(node[node >= 0], return_inverse=True)[1]).max() <= 40  # small buckets
    assert 3000 < len(np.unique(ls["side1"]["node"])) <= BP.LONG_NODES + 1 and any(x["occupied"].any() for x in ls["side2"])
    lr = BP.batch("long_robust")
    assert lr["kind"] == "tri" and lr["side1"]["node"] is None and all(x["node"] is None for x in lr["side2"])
    assert len(lr["side1"]["desc"]) == lim + 1 and [len(x["desc"]) for x in lr["side2"]] == [500, 0]


# ---- the batched logic, restated: all sides ordered by (node, index); a row's bucket is the equal range of its node inside ITS
# problem's side-2 segment of the concatenated order; per problem an owner table of its own.  `shared_owner`: one owner table for all
# problems of a shared side 2; `ignore_boundary`: the bucket lookup runs over the whole concatenation.
def _hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def restated(b, ori, shared_owner=False, ignore_boundary=False):
    assert b["kind"] == "bow"
    k = BP.num_problems(b)
    lowe = np.float32(b["lowe_ratio"])
    shared2 = isinstance(b["side2"], dict)
    segs, keys, owner_of = [], [], {}
    for p in range(k):  # the concatenated (node, index) order of every problem's side 2
        _, s2 = BP.sides(b, p)
        node = np.asarray(s2["node"], np.int64)
        order = np.lexsort((np.arange(len(node)), np.where(node < 0, 1 << 40, node)))
        segs.append(order)
        keys.append(np.where(node < 0, 1 << 40, node)[order])
    cat_keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    cat_prob = np.concatenate([np.full(len(x), p) for p, x in enumerate(segs)]) if segs else np.zeros(0, np.int64)
    cat_idx = np.concatenate(segs) if segs else np.zeros(0, np.int64)
    out = []
    for p in range(k):
        s1, s2 = BP.sides(b, p)
        n1 = len(s1["desc"])
        match = np.full(n1, -1, np.int32)
        owner = owner_of.setdefault(0 if (shared_owner and shared2) else p, set())
        node1 = np.asarray(s1["node"], np.int64)
        v1, v2, occ = BP._valid(s1), BP._valid(s2), s2.get("occupied")
        for q in np.lexsort((np.arange(n1), np.where(node1 < 0, 1 << 40, node1))):
            if node1[q] < 0 or (v1 is not None and not v1[q]):
                continue
            if ignore_boundary:
                cand = [(int(cat_prob[i]), int(cat_idx[i])) for i in np.flatnonzero(cat_keys == node1[q])]
                cand = [j for pp, j in cand if pp == p or j < len(s2["desc"])]  # (a foreign index that happens to exist here is used as if its own)
            else:
                cand = [int(j) for j in segs[p][keys[p] == node1[q]]]
            best, second, best_j = 256, 256, -1
            for j in cand:
                if (v2 is not None and not v2[j]) or (occ is not None and occ[j]) or j in owner:
                    continue
                if ori:
                    d = np.float32(s1["angle"][q]) - np.float32(s2["angle"][j])
                    d = d + np.float32(360) if d <= -180 else d
                    d = d - np.float32(360) if d > 180 else d
                    if abs(d) > 30:
                        continue
                h = _hamming(s1["desc"][q], s2["desc"][j])
                if h < best:
                    second, best, best_j = best, h, j
                elif h < second:
                    second = h
            if best_j < 0 or best > 50 or np.float32(lowe * np.float32(second)) < np.float32(best):
                continue
            match[q] = best_j
            owner.add(best_j)
        out.append((match, int((match >= 0).sum())))
    return out


BOW_SMALL = ["reloc", "loop", "unshared", "planted_eq", "many"]


def _differs(a, b):
    return any(not np.array_equal(x[0], y[0]) or x[1] != y[1] for x, y in zip(a, b))


@pytest.fixture(scope="module")
def light():
    """The bow classes cut down to what plain Python walks in seconds: at most 6 problems each."""
    out = {}
    for name in BOW_SMALL:
        b = dict(BP.batch(name))
        for key in ("side1", "side2"):
            if not isinstance(b[key], dict):
                b[key] = list(b[key])[:6]
        if name == "planted_eq":  # without the 1 100-query chain and the 1 024 / 1 025 buckets
            keep = [p for p in range(len(b["side1"])) if len(b["side1"][p]["desc"]) * len(b["side2"][p]["desc"]) < 5000][:6]
            b["side1"], b["side2"] = [BP.batch(name)["side1"][p] for p in keep], [BP.batch(name)["side2"][p] for p in keep]
        out[name] = b
    return out


def test_restatement_agrees_and_wrong_variants_are_caught(light):
    caught_owner = caught_boundary = False
    for name, b in light.items():
        ref = BP.oracle(b, True)
        assert not _differs(restated(b, True), ref), name
        caught_owner = caught_owner or _differs(restated(b, True, shared_owner=True), ref)
        caught_boundary = caught_boundary or _differs(restated(b, True, ignore_boundary=True), ref)
    assert caught_owner, "no class tells a shared owner table from per-problem ones"
    assert caught_boundary, "no class tells a bucket lookup that ignores the problem boundary"


def test_header_additions():
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    assert re.search(r"#define\s+SVGPU_ABI_VERSION\s+1\b", hdr)
    from stella_vslam_amd._lib import parse_header
    sigs = parse_header(hdr)
    assert len(sigs["svgpu_bow_match_batch"][1]) == 10 and len(sigs["svgpu_match_for_triangulation_batch"][1]) == 16
    body = re.search(r"typedef struct svgpu_match_view \{(.*?)\} svgpu_match_view;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == ["desc", "angle", "valid", "node", "octave", "bearings", "xright", "occupied", "n"]


def test_bucket_batch_arena_layout(tmp_path):
    out = build_and_run("bucket_batch_arena_check.cpp", "bucket batch arena ok", tmp_path)
    assert out.count("ok ") >= 50
