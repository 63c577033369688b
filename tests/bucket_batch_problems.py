"""Batches for the batched bucket matchers (svgpu_bow_match_batch, svgpu_match_for_triangulation_batch): numpy and the CPU oracle only.

A batch is a dict: kind ('bow' | 'tri'), side1 / side2 (a list of side dicts, or ONE dict = shared by every problem), lowe_ratio, for
'tri' also E_12 (K x 3 x 3), epipole_in_2 (K x 3), valid_epipole (K), scale_factors, residual_rad_thr, and for the planted classes
`expect(check_orientation)`: the designed per-problem answers.  Side dicts use the keywords of stella_vslam_amd.match's batch wrappers
(desc, angle, valid | has_lm, node, octave, bearings, xright, occupied).  The expected result of a batch is the list of the single
oracle's per-problem results (`oracle`): the oracle itself knows nothing of batches.

Scene classes come from tests/match_problems.py; in the planted classes a target is a query with exactly d bits flipped, so every
distance is set by hand (tests/cand_problems.py does the same for the candidate matcher)."""
import functools

import numpy as np

from oracle import oracle as O
from tests import match_problems as MP

CLASSES = ["reloc", "loop", "unshared", "tri_bow", "tri_robust", "planted_eq", "planted_lo", "planted_hi", "planted_tri", "spill", "many", "long_sides",
           "long_robust"]
REGIME_BUCKETS = (64, 65, 1024, 1025)   # at most one entry per lane / the LDS sort / its limit / unsorted
CHAIN = 1100                            # live queries whose claims chain across the replay's 1 024-query chunk


def num_problems(b):
    return len(b["side2"]) if isinstance(b["side1"], dict) else len(b["side1"])


def sides(b, p):
    s1 = b["side1"] if isinstance(b["side1"], dict) else b["side1"][p]
    s2 = b["side2"] if isinstance(b["side2"], dict) else b["side2"][p]
    return s1, s2


def _valid(s):
    if s.get("valid") is not None or s.get("has_lm") is None:
        return s.get("valid")
    return (np.asarray(s["has_lm"]) == 0).astype(np.uint8)


def single(b, p, check_orientation, bow_match, tri_match):
    """Problem p through a SINGLE matcher: bow_match / tri_match are the oracle's functions or thin wrappers of the library's single calls
    with the oracle's signatures (lowe_ratio, check_orientation, ...)."""
    s1, s2 = sides(b, p)
    if b["kind"] == "bow":
        return bow_match(b["lowe_ratio"], check_orientation, s1["desc"], s1.get("angle"), _valid(s1), s1.get("node"), s2["desc"], s2.get("angle"),
                         s2.get("node"), valid2=_valid(s2), occupied2=s2.get("occupied"))
    inv = lambda s: None if _valid(s) is None else (np.asarray(_valid(s)) == 0).astype(np.uint8)  # noqa: E731  (back to has_lm)
    return tri_match(b["lowe_ratio"], check_orientation, s1["desc"], s1.get("angle"), s1["octave"], s1["bearings"], inv(s1), s2["desc"], s2.get("angle"),
                     s2["bearings"], inv(s2), b["E_12"][p], b["epipole_in_2"][p], int(b["valid_epipole"][p]), b["scale_factors"], b["residual_rad_thr"],
                     xright1=s1.get("xright"), xright2=s2.get("xright"), node1=s1.get("node"), node2=s2.get("node"))


def oracle(b, check_orientation):
    """[(match array, count)] per problem, from the single CPU oracle."""
    out = []
    for p in range(num_problems(b)):
        s1, _ = sides(b, p)
        if len(s1["desc"]) == 0:
            out.append((np.zeros(0, np.int32), 0))
            continue
        m, n = single(b, p, check_orientation, O.bow_match, O.match_for_triangulation)
        out.append((m, int(n)))
    return out


def reversed_batch(b):
    r = dict(b)
    for k in ("side1", "side2"):
        if not isinstance(b[k], dict):
            r[k] = list(b[k])[::-1]
    for k in ("E_12", "epipole_in_2", "valid_epipole"):
        if k in b:
            r[k] = np.ascontiguousarray(np.asarray(b[k])[::-1])
    return r


def unshared_batch(b):
    """The same batch with its shared side passed K times."""
    r, k = dict(b), num_problems(b)
    for key in ("side1", "side2"):
        if isinstance(b[key], dict):
            r[key] = [b[key]] * k
    return r


def batch_of_one(b, p):
    r = dict(b)
    s1, s2 = sides(b, p)
    r["side1"], r["side2"] = [s1], [s2]
    for k in ("E_12", "epipole_in_2", "valid_epipole"):
        if k in b:
            r[k] = np.ascontiguousarray(np.asarray(b[k])[p:p + 1])
    return r


# ------------------------------------------------------------------------------------------------ scenes
def _take(side, idx):
    return {k: (None if v is None else np.ascontiguousarray(np.asarray(v)[idx])) for k, v in side.items()}


def _bow_sides(seed, keyframes=False):
    kw = MP.bow(MP.scene(seed=seed), seed=seed + 1, keyframes=keyframes)
    s1 = dict(desc=kw["desc1"], angle=kw["angle1"], valid=kw["valid1"], node=kw["node1"])
    s2 = dict(desc=kw["desc2"], angle=kw["angle2"], valid=kw.get("valid2"), node=kw["node2"], occupied=kw.get("occupied2"))
    return s1, s2


@functools.lru_cache(maxsize=None)
def batch(name):
    return globals()["_" + name]()


def _reloc():
    """6 keyframes against ONE frame (side 2 shared): 0 plain, 1 and 2 the same arrays, 3 valid all zero, 4 empty, 5 nodes disjoint from
    the frame's; the frame has occupied keypoints."""
    rng = np.random.default_rng(11)
    s1, frame = _bow_sides(7)
    n = len(s1["desc"])
    sub = lambda m: _take(s1, np.sort(rng.choice(n, m, replace=False)))  # noqa: E731
    k0, k1 = sub(n), sub(n * 2 // 3)
    k3 = sub(n // 2)
    k3["valid"] = np.zeros(len(k3["desc"]), np.uint8)
    k4 = _take(s1, np.zeros(0, np.int64))
    k5 = sub(n // 3)
    k5["node"] = (k5["node"] + 100000).astype(np.int32)
    assert frame["occupied"] is not None and frame["occupied"].any()
    return dict(kind="bow", lowe_ratio=0.75, side1=[k0, k1, k1, k3, k4, k5], side2=frame, degenerate=(3, 4, 5))


def _loop():
    """ONE keyframe (side 1 shared) against 5 candidates of different sizes, n2 == 1 among them; valid2 present."""
    rng = np.random.default_rng(12)
    cur, other = _bow_sides(9, keyframes=True)
    n = len(other["desc"])
    live = np.flatnonzero(other["valid"])
    cands = [_take(other, np.sort(rng.choice(n, m, replace=False))) for m in (n, n // 2, 333, 65)] + [_take(other, live[:1])]
    assert all(c["valid"] is not None for c in cands)
    return dict(kind="bow", lowe_ratio=0.75, side1=cur, side2=cands, degenerate=(4,))


def _unshared():
    """3 problems, nothing shared, sizes 1, 64 and 700."""
    rng = np.random.default_rng(13)
    s1, s2 = _bow_sides(21)
    n1, n2 = len(s1["desc"]), len(s2["desc"])
    a1, a2 = [], []
    for m in (1, 64, 700):
        a1.append(_take(s1, np.sort(rng.choice(n1, m, replace=False))))
        a2.append(_take(s2, np.sort(rng.choice(n2, m, replace=False))))
    # the one-keypoint problem: the same landmark's keypoint on both sides cannot be chosen blindly; it only has to be well-formed
    return dict(kind="bow", lowe_ratio=0.75, side1=a1, side2=a2, degenerate=(0,))


def _tri(with_nodes):
    """ONE keyframe against 4 neighbours with per-problem E_12; valid_epipole mixed; the stereo scene has x_right on some keypoints."""
    rng = np.random.default_rng(14)
    sc = MP.scene(seed=7, stereo=True)
    ocam = MP.make_cams(sc, "oracle")
    kw = MP.triangulation(sc, lambda R, t, c: O.reproject_to_bearing(ocam, R, t, c), with_nodes=with_nodes)
    s1 = dict(desc=kw["desc1"], angle=kw["angle1"], octave=kw["octave1"], bearings=kw["bearings1"], has_lm=kw["has_lm1"], xright=kw["xright1"],
              node=kw.get("node1"))
    full = dict(desc=kw["desc2"], angle=kw["angle2"], bearings=kw["bearings2"], has_lm=kw["has_lm2"], xright=kw["xright2"], node=kw.get("node2"))
    assert (np.asarray(full["xright"]) >= 0).any() and (np.asarray(full["xright"]) < 0).any()
    n2 = len(full["desc"])
    nb = [full] + [_take(full, np.sort(rng.choice(n2, m, replace=False))) for m in (n2 * 3 // 4, n2 // 2, 200)]
    E = np.stack([np.asarray(kw["E_12"], np.float64) * s for s in (1.0, 1.0, 2.0, 1.0)])
    E[3] = E[3] + 1e-3 * rng.normal(0, 1, (3, 3))  # a slightly wrong geometry: fewer pairs pass, still a well-formed problem
    epi = np.stack([np.asarray(kw["epipole_in_2"], np.float64)] * 4)
    return dict(kind="tri", lowe_ratio=0.8, side1=s1, side2=nb, E_12=E, epipole_in_2=epi, valid_epipole=np.array([1, 0, 1, 0], np.int32),
                scale_factors=kw["scale_factors"], residual_rad_thr=kw["residual_rad_thr"], degenerate=())


def _tri_bow():
    return _tri(True)


def _tri_robust():
    return _tri(False)


def acos_margin(b):
    """Smallest distance, over all pairs of a 'tri' batch, between the epipolar residual and its threshold, and between the epipole cosine
    and its cut-off, in units of the quantity's own rounding (the GPU test asserts that no pair sits within rounding distance)."""
    worst = np.inf
    for p in range(num_problems(b)):
        s1, s2 = sides(b, p)
        b1, b2 = np.asarray(s1["bearings"], np.float64), np.asarray(s2["bearings"], np.float64)
        if len(b1) == 0 or len(b2) == 0:  # no pairs
            continue
        e = b2 @ np.asarray(b["E_12"][p], np.float64).T                      # rows: E b2
        cosr = np.clip((b1 @ e.T) / np.linalg.norm(e, axis=1)[None, :], -1, 1)
        res = np.abs(np.pi / 2 - np.arccos(cosr))
        thr = (np.asarray(b["scale_factors"], np.float32)[np.asarray(s1["octave"])] * np.float32(b["residual_rad_thr"])).astype(np.float64)
        worst = min(worst, np.abs(res - thr[:, None]).min() / 1e-15)
        if b["valid_epipole"][p]:
            worst = min(worst, np.abs(b2 @ np.asarray(b["epipole_in_2"][p], np.float64) - 0.99862953475).min() / 1e-15)
    return worst


# ------------------------------------------------------------------------------------------------ planted
def _bits(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(desc, d, rng, avoid=()):
    """`desc` (32 bytes) with exactly d bits flipped, none of them in `avoid`."""
    free = np.setdiff1d(np.arange(256), np.asarray(avoid, np.int64))
    out = desc.copy()
    for bit in rng.choice(free, d, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def _side(desc, angle=None, node=None, **kw):
    n = len(desc)
    s = dict(desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32), angle=np.zeros(n, np.float32) if angle is None else np.asarray(angle, np.float32),
             node=np.zeros(n, np.int32) if node is None else np.asarray(node, np.int32))
    s.update(kw)
    return s


def _planted_problems(rng, tri):
    """[(side1, side2, expect(check_orientation))] -- every problem one bucket (node 0).  RATIO (bow): accept best <= 50 unless
    lowe * second < best.  TRIANGULATION: a candidate counts only when d < the running best, which starts AT 50 (strict), and second is
    the last superseded best (256 when the first candidate in scan order is the best one)."""
    P = []
    far = lambda q: _flip(q, 200, rng)  # noqa: E731
    q = _bits(rng, 1)[0]
    # best == 50: RATIO accepts, TRIANGULATION (strict) does not; best == 49 is accepted by RATIO
    P.append((_side([q]), _side([_flip(q, 50, rng), far(q)]), lambda ori: [-1] if tri else [0]))
    # (TRIANGULATION: the superseded "best" is the initial 50, and 0.75 * 50 < 49 fails the ratio test)
    P.append((_side([q]), _side([far(q), _flip(q, 49, rng)]), lambda ori: [-1] if tri else [1]))
    P.append((_side([q]), _side([_flip(q, 51, rng), far(q)]), lambda ori: [-1]))
    # the Lowe test with best = 36 and second = 48: lowe * 48 against 36 (the class sets lowe to 0.75 and its two fp32 neighbours).
    # Scan order second-then-best makes 48 the superseded best in TRIANGULATION too.
    P.append((_side([q]), _side([_flip(q, 48, rng), _flip(q, 36, rng)]), "lowe"))
    # |angle difference| exactly 30 passes (the gate is > 30), the next float does not: the query falls back to the farther target
    t30 = _side([_flip(q, 10, rng), _flip(q, 20, rng)], angle=[30.0, 0.0])
    t30p = _side([_flip(q, 10, rng), _flip(q, 20, rng)], angle=[np.nextafter(np.float32(30), np.float32(40)), 0.0])
    P.append((_side([q]), t30, lambda ori: [0]))
    P.append((_side([q]), t30p, lambda ori: [1] if ori else [0]))
    # a target wanted by two queries: the earlier one takes it, the later one its own second choice
    q2 = _flip(q, 4, rng)
    t0 = _flip(q, 6, rng)
    P.append((_side([q, q2]), _side([t0, far(q), _flip(q2, 30, rng)]), "oracle"))
    if not tri:  # an initially occupied best (bow only: the triangulation matchers have no such input)
        P.append((_side([q]), _side([_flip(q, 5, rng), _flip(q, 30, rng)], occupied=np.array([1, 0], np.uint8)), lambda ori: [1]))
    # the regimes of the distance kernel: one query, a bucket of exactly 64 / 65 / 1 024 / 1 025 side-2 keypoints in its node, the planted
    # best last; keypoints of another node around it
    for m in REGIME_BUCKETS:
        t = _bits(rng, m + 7)
        node = np.concatenate([np.zeros(m, np.int32), np.full(7, 5, np.int32)])
        t[m - 1] = _flip(q, 5, rng)
        perm = rng.permutation(m + 7)
        P.append((_side([q]), _side(t[perm], node=node[perm]), (lambda at: lambda ori: [at])(int(np.flatnonzero(perm == m - 1)[0]))))
    # CHAIN queries whose claims displace each other one by one across the replay's chunk of 1 024: b_{i+1} = b_i with 20 bits flipped
    # (disjoint from the step before: next-but-one neighbours are exactly 40 apart), query 0 = b_1, query i = b_i, target i = b_{i+1}.
    # Query 0 takes target 0 at distance 0; query i finds its own (target i - 1) taken and takes target i at 20 (second: 40).
    b = [_bits(rng, 1)[0]]
    prev = []
    for _ in range(CHAIN + 1):
        step = rng.choice(np.setdiff1d(np.arange(256), prev), 20, replace=False)
        nxt = b[-1].copy()
        for bit in step:
            nxt[bit >> 3] ^= np.uint8(1 << (bit & 7))
        b.append(nxt)
        prev = step
    qs = np.stack([b[1]] + [b[i] for i in range(1, CHAIN)])
    ts = np.stack([b[i + 1] for i in range(CHAIN)])
    P.append((_side(qs), _side(ts), lambda ori: list(range(CHAIN))))
    return P


def _planted(lowe, tri=False):
    rng = np.random.default_rng(15)
    lowe = np.float32(lowe)
    P = _planted_problems(rng, tri)
    accept = not (np.float32(lowe * np.float32(48)) < np.float32(36))
    s1, s2, ex = [], [], []
    for a, c, e in P:
        if tri:  # a geometry that admits every pair exactly: E = [t]x with t = x, all bearings = z: (E b2) . b1 = 0, acos(0) = pi / 2
            for s in (a, c):
                s["bearings"] = np.tile(np.array([0.0, 0.0, 1.0]), (len(s["desc"]), 1))
            a["octave"] = np.zeros(len(a["desc"]), np.int32)
        s1.append(a), s2.append(c)
        ex.append(e)

    def expect(ori):
        out = []
        for p, e in enumerate(ex):
            if e == "oracle":
                out.append(None)
            elif e == "lowe":
                out.append(np.array([1 if accept else -1], np.int32))
            else:
                out.append(np.array(e(ori), np.int32))
        return out
    bt = dict(kind="tri" if tri else "bow", lowe_ratio=float(lowe), side1=s1, side2=s2, expect=expect, degenerate=())
    if tri:
        k = len(P)
        E = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])
        bt.update(E_12=np.stack([E] * k), epipole_in_2=np.tile(np.array([1.0, 0, 0]), (k, 1)), valid_epipole=np.zeros(k, np.int32),
                  scale_factors=np.array([1.0, 1.2], np.float32), residual_rad_thr=0.01)
    return bt


def _planted_eq():
    return _planted(0.75)


def _planted_lo():
    return _planted(np.nextafter(np.float32(0.75), np.float32(0)))


def _planted_hi():
    return _planted(np.nextafter(np.float32(0.75), np.float32(1)))


def _planted_tri():
    return _planted(0.75, tri=True)


# ------------------------------------------------------------------------------------------------ sizes
SPILL_N = 11000  # cand_lds_bytes(11000, 11000, 0) = 165 016 bytes > the 153 600-byte budget: the replay's tables go to global memory


def _small(rng, n=64):
    q = _bits(rng, n)
    t = np.stack([_flip(q[i], int(rng.integers(0, 30)), rng) for i in range(n)])
    perm = rng.permutation(n)
    node = (np.arange(n) % 8).astype(np.int32)
    return _side(q, angle=rng.uniform(0, 360, n), node=node, valid=(rng.uniform(0, 1, n) < 0.9).astype(np.uint8)), \
        _side(t[perm], angle=rng.uniform(0, 360, n), node=node[perm])


def _spill():
    """One 11 000 x 11 000 problem (few shared nodes: most keypoints sit in nodes the other side lacks) between two small ones."""
    rng = np.random.default_rng(16)
    n, m = SPILL_N, 600   # m planted pairs spread over 40 shared nodes; everything else in nodes of its own side
    q, t = _bits(rng, n), _bits(rng, n)
    node1, node2 = (1000 + rng.integers(0, 500, n)).astype(np.int32), (5000 + rng.integers(0, 500, n)).astype(np.int32)
    qi, ti = rng.choice(n, m, replace=False), rng.choice(n, m, replace=False)
    for a, c in zip(qi, ti):
        t[c] = _flip(q[a], int(rng.integers(0, 40)), rng)
        node1[a] = node2[c] = int(rng.integers(0, 40))
    big1 = _side(q, angle=rng.uniform(0, 360, n), node=node1)
    big2 = _side(t, angle=rng.uniform(0, 360, n), node=node2)
    a1, a2 = _small(rng)
    b1, b2 = _small(rng)
    return dict(kind="bow", lowe_ratio=0.75, side1=[a1, big1, b1], side2=[a2, big2, b2], degenerate=())


def _many():
    """300 copies of one 64 x 64 problem: more problems than compute units."""
    s1, s2 = _small(np.random.default_rng(17))
    return dict(kind="bow", lowe_ratio=0.75, side1=[s1] * 300, side2=[s2] * 300, degenerate=())


# ------------------------------------------------------------------------------------------------ sides beyond the one-workgroup sort
SORT_SMALL_MAX = 16384                    # SV_SORT_SMALL_MAX of csrc/sv_sort.h: longer sides take the radix sort, n1 beyond it the long scan
LONG_SHARED, LONG_OTHERS = 20000, (16385, 300, 16384, 0)
LONG_NODES = 4000                         # distinct node ids: buckets of about 5, so that the Python-driven oracle stays fast


def _long_nodes(rng, ids, n):
    node = ids[rng.integers(0, len(ids), n)].astype(np.int32)
    node[rng.uniform(0, 1, n) < 0.05] = -1
    return node


def _long_sides():
    """ONE keyframe of 20 000 keypoints (side 1, shared) against candidates of 16 385, 300, 16 384 and 0 keypoints: sides on both sides of
    the one-workgroup sort's limit in one batch, every single call with n1 beyond the short scan.  Node ids from 4 000 values, some -1;
    planted pairs (a target = a query with a few bits flipped, in the query's node, at the query's angle) give every non-empty problem matches."""
    rng = np.random.default_rng(18)
    ids = rng.integers(0, 1 << 31, LONG_NODES, dtype=np.int64)
    n1 = LONG_SHARED
    q, node1 = _bits(rng, n1), _long_nodes(rng, ids, n1)
    s1 = _side(q, angle=rng.uniform(0, 360, n1), node=node1, valid=(rng.uniform(0, 1, n1) < 0.9).astype(np.uint8))
    with_node = np.flatnonzero(node1 >= 0)
    cands = []
    for n2 in LONG_OTHERS:
        t, node2, angle2 = _bits(rng, n2), _long_nodes(rng, ids, n2), rng.uniform(0, 360, n2).astype(np.float32)
        m = min(n2, 1200) // 3
        for a, c in zip(rng.choice(with_node, m, replace=False), rng.choice(n2, m, replace=False) if n2 else []):
            t[c] = _flip(q[a], int(rng.integers(0, 40)), rng)
            node2[c], angle2[c] = node1[a], s1["angle"][a]
        cands.append(_side(t, angle=angle2, node=node2, occupied=(rng.uniform(0, 1, n2) < 0.02).astype(np.uint8)))
    return dict(kind="bow", lowe_ratio=0.75, side1=s1, side2=cands, degenerate=(3,))


LONG_ROBUST_N1, LONG_ROBUST_OTHERS = 16385, (500, 0)


def _long_robust():
    """The triangulation matcher without node ids (match::robust: one bucket, identity order) with a shared side 1 of 16 385 keypoints: the
    identity order beyond the one-workgroup sort and, in the single call, the long scan.  The geometry of planted_tri admits every pair
    exactly, so the Hamming cut-off alone thins the 16 385 x 500 pairs; 150 planted pairs match."""
    rng = np.random.default_rng(19)
    n1 = LONG_ROBUST_N1
    q = _bits(rng, n1)
    s1 = _side(q, angle=rng.uniform(0, 360, n1), octave=np.zeros(n1, np.int32))
    s1["node"] = None
    cands = []
    for n2 in LONG_ROBUST_OTHERS:
        t, angle2 = _bits(rng, n2), rng.uniform(0, 360, n2).astype(np.float32)
        m = n2 * 3 // 10
        for a, c in zip(rng.choice(n1, m, replace=False), rng.choice(n2, m, replace=False) if n2 else []):
            t[c] = _flip(q[a], int(rng.integers(0, 30)), rng)
            angle2[c] = s1["angle"][a]
        c2 = _side(t, angle=angle2)
        c2["node"] = None
        cands.append(c2)
    for s in [s1] + cands:
        s["bearings"] = np.tile(np.array([0.0, 0.0, 1.0]), (len(s["desc"]), 1))
    k = len(cands)
    E = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    return dict(kind="tri", lowe_ratio=0.8, side1=s1, side2=cands, E_12=np.stack([E] * k), epipole_in_2=np.tile(np.array([1.0, 0, 0]), (k, 1)),
                valid_epipole=np.zeros(k, np.int32), scale_factors=np.array([1.0, 1.2], np.float32), residual_rad_thr=0.01, degenerate=(1,))
