"""Planted problems for robust::brute_force_match (match/robust.cc:232-328): descriptor sets whose Hamming distances are set bit by bit, so
that the decisions of the matcher land exactly on its boundaries -- best distance 50 / 51, lowe_ratio * second == best in fp32, second
distances at the listing cutoff dmax of the HIP matcher, ties, extreme popcounts, the +-30 degree orientation gate with wrap-around and
non-finite angles, claim chains that need one replay sweep per query, and valid2 masks.  numpy + the CPU oracle only.

A case is (d1, a1, d2, a2, valid2) plus the lowe_ratio / check_orientation it is meant for; side 1 is the scanned (frame) side, side 2
the queries (keyframe keypoints).  The generators verify their plants with O.hamming_matrix and reseed when the random background
would undercut them."""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle import oracle as O

F32 = np.float32
NAN = float("nan")


@dataclasses.dataclass
class Case:
    name: str
    d1: np.ndarray
    a1: np.ndarray
    d2: np.ndarray
    a2: np.ndarray
    valid2: np.ndarray | None
    ratio: float
    check: bool
    info: dict = dataclasses.field(default_factory=dict)  # what the class planted (read by the class tests)

    def args(self):
        return self.d1, self.a1, self.d2, self.a2, self.valid2

    def oracle(self):
        return O.brute_force_match(self.d1, self.a1, self.d2, self.a2, self.valid2, self.ratio, self.check)


def dmax_of(ratio: float) -> int:
    """The listing cutoff of the HIP matcher (sv_launch_bf): candidates farther than this can never decide."""
    r = F32(ratio)
    if r > 0 and F32(F32(50.0) / r) + F32(2.0) < F32(256.0):
        d = int(F32(50.0) / r) + 2
    else:
        d = 256
    return max(d, 50)


def accepts(best: int, second: int, ratio: float) -> bool:
    """the ratio test of robust.cc in fp32: rejected iff lowe_ratio * second < best"""
    return not (F32(ratio) * F32(second) < F32(best))


# ---------------------------------------------------------------------------------------------------- bits
def _bits(rng, k, allowed=None):
    pool = np.arange(256) if allowed is None else np.asarray(sorted(allowed))
    return rng.choice(pool, k, replace=False)


def flip(desc, bits):
    out = desc.copy()
    for b in np.asarray(bits, int):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def at_distance(rng, desc, k, allowed=None):
    """a descriptor exactly k bits away from `desc`"""
    return flip(desc, _bits(rng, k, allowed))


def from_bits(bits):
    return flip(np.zeros(32, np.uint8), bits)


def popcount(d):
    return np.unpackbits(np.atleast_2d(d), axis=1).sum(1)


def _rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _angles(rng, n):
    return rng.uniform(0, 360, n).astype(np.float32)


def _verify(d1, d2, plants, floor):
    """plants {(j, i): distance} hold, and every other target of query j is at least floor[j] away"""
    D = O.hamming_matrix(d1, d2).astype(int)
    for (j, i), d in plants.items():
        if D[j, i] != d:
            return False
    for j, f in floor.items():
        planted = {i for (jj, i) in plants if jj == j}
        others = [i for i in range(len(d1)) if i not in planted]
        if others and D[j, others].min() < f:
            return False
    return True


def _retry(make, seed, tries=40):
    for t in range(tries):
        out = make(np.random.default_rng(seed * 1000 + t))
        if out is not None:
            return out
    raise RuntimeError("could not plant the problem without the background undercutting it")


# ---------------------------------------------------------------------------------------------------- 1. HAMMING_DIST_THR_LOW = 50
def threshold(seed=1, check=True):
    """Queries with a planted best at 49, 50 or 51 and a clear second: the background, or a planted one at 67 (listed under the MFMA
    cutoff dmax(0.75) = 68, accepted by the ratio test).  best <= 50 matches; 51 never does."""
    bests = [49, 50, 51] * 8
    seconds = [None, 67] * 12

    def make(rng):
        n2 = len(bests)
        n1 = 2 * n2 + 40
        d2, d1 = _rand(rng, n2), _rand(rng, n1)
        slots = rng.permutation(n1)
        plants, floor, best_of = {}, {}, {}
        for j, (b, s) in enumerate(zip(bests, seconds)):
            ib = int(slots[2 * j])
            d1[ib] = at_distance(rng, d2[j], b)
            plants[(j, ib)] = b
            best_of[j] = (ib, b)
            if s is not None:
                isx = int(slots[2 * j + 1])
                d1[isx] = at_distance(rng, d2[j], s)
                plants[(j, isx)] = s
            floor[j] = 80 if s is None else 68
        if not _verify(d1, d2, plants, floor):
            return None
        return Case(f"threshold/ori{int(check)}", d1, np.full(n1, 123.5, np.float32), d2, np.full(n2, 123.5, np.float32), None, 0.75, check,
                    {"best": best_of})
    return _retry(make, seed)


# ---------------------------------------------------------------------------------------------------- 2. lowe_ratio * second == best
# (best, second, ratio) with float(ratio) * second == best in fp32: exactly, or by rounding onto best (0.8f * 40, 0.9f * 50)
RATIO_EQUALITIES = [(30, 40, 0.75), (25, 50, 0.5), (21, 42, 0.5), (36, 48, 0.75), (32, 40, 0.8), (40, 50, 0.8), (45, 50, 0.9)]


def ratio_equality(seed=2):
    """Each (best, second, ratio) at that ratio and one ulp below / above it.  The ratio test alone decides: no claims, second listed."""
    cases = []
    for k, (b, s, r) in enumerate(RATIO_EQUALITIES):
        assert F32(r) * F32(s) == F32(b), (b, s, r)

        def make(rng, b=b, s=s):
            n1, n2 = 48, 3
            d2, d1 = _rand(rng, n2), _rand(rng, n1)
            d1[7] = at_distance(rng, d2[1], s)   # the second first in index order: the scan meets it before the best
            d1[29] = at_distance(rng, d2[1], b)
            if not _verify(d1, d2, {(1, 7): s, (1, 29): b}, {1: s + 15, 0: 70, 2: 70}):
                return None
            return d1, _angles(rng, n1), d2, _angles(rng, n2)
        d1, a1, d2, a2 = _retry(make, seed * 100 + k)
        for tag, rr in (("eq", F32(r)), ("down", np.nextafter(F32(r), F32(0))), ("up", np.nextafter(F32(r), F32(1)))):
            assert s <= dmax_of(float(rr))
            cases.append(Case(f"ratio_{b}_{s}_{r}_{tag}", d1, a1, d2, a2, None, float(rr), False,
                              {"query": 1, "target": 29, "best": b, "second": s, "accept": accepts(b, s, float(rr)), "tag": tag}))
    return cases


# ---------------------------------------------------------------------------------------------------- 3. around dmax
def around_dmax(seed=3):
    """Seconds planted at dmax, dmax + 1 and dmax + 2 (the last listed distance and the first unlisted ones) for lowe_ratios 0.5 .. 1.5;
    the MFMA / VALU kernel switch (0.40: dmax 127, about half of all random pairs are candidates, so every row overflows its 16 slots;
    0.39: dmax 130, the VALU kernel); the degenerate ratios 0, negative and NaN (dmax 256: the whole row is listed)."""
    cases = []
    for k, r in enumerate([0.5, 0.6, 0.75, 0.8, 1.0, 1.5]):
        dm = dmax_of(r)

        def make(rng, dm=dm, r=r):
            n2, n1 = 9, 64
            d2, d1 = _rand(rng, n2), _rand(rng, n1)
            plants, floor, sec = {}, {}, {}
            for j in range(n2):
                s, bst = dm + j % 3, [50, 48, 40][j // 3]
                d1[2 * j] = at_distance(rng, d2[j], s)
                d1[2 * j + 21] = at_distance(rng, d2[j], bst)
                plants[(j, 2 * j)] = s
                plants[(j, 2 * j + 21)] = bst
                floor[j] = s + 1
                sec[j] = (s, bst)
            if not _verify(d1, d2, plants, floor):
                return None
            return Case(f"dmax_r{r}", d1, np.full(n1, 200.0, np.float32), d2, np.full(n2, 190.0, np.float32), None, r, True,
                        {"dmax": dm, "planted": sec})
        cases.append(_retry(make, seed * 100 + k))
    # the kernel switch and the degenerate ratios on random + planted rows (noisy copies, exact copies, duplicated targets)
    rng = np.random.default_rng(seed)
    n1, n2 = 600, 300
    d1 = _rand(rng, n1)
    src = rng.integers(0, n1 - 20, n2)
    d2 = d1[src].copy()
    for j in range(n2):
        if j % 5:
            d2[j] = at_distance(rng, d2[j], int(rng.integers(1, 60)))
    d1[n1 - 20:] = d1[src[:20]]  # duplicated targets: second == best for some exact-copy queries
    a1 = _angles(rng, n1)
    a1[n1 - 20:] = a1[src[:20]]
    a2 = ((a1[src] + rng.normal(0, 12, n2)) % 360).astype(np.float32)
    for r in (0.40, 0.39, 0.0, -0.5, NAN):
        cases.append(Case(f"ratio_{r}", d1, a1, d2, a2, None, r, True, {"dmax": dmax_of(r)}))
    return cases


# ---------------------------------------------------------------------------------------------------- 4. ties
def ties(seed=4):
    cases = []
    # (a) the same best distance in several angle bins: the lowest ORIGINAL idx_1 wins, whatever the angle-sorted order
    rng = np.random.default_rng(seed)
    n1, n2 = 80, 6
    d2, d1 = _rand(rng, n2), _rand(rng, n1)
    a2 = np.array([100.0, 5.0, 355.0, 180.0, 100.0, 20.0], np.float32)
    a1 = _angles(rng, n1)
    perm = rng.permutation(n1)
    win = {}
    for j in range(n2):
        idx = sorted(perm[5 * j:5 * j + 5].tolist())
        while True:  # the lowest index must not sit in the lowest bin
            offs = rng.permutation([29.5, -12.0, 0.0, 14.0, -29.0])
            bins = np.floor(F32((a2[j] + offs) % 360)).astype(int)
            if bins[0] != bins.min():
                break
        for i, o in zip(idx, offs):
            d1[i] = at_distance(rng, d2[j], 20)
            a1[i] = F32((a2[j] + o) % 360)
        win[j] = idx[0]
    cases.append(Case("tie_bins", d1, a1, d2, a2, None, 1.0, True, {"winner": win}))
    # (b) more than 16 candidates at one distance (a list keeps 16): 20 targets 30 bits from one query
    rng = np.random.default_rng(seed + 1)
    n1, n2 = 90, 4
    d2, d1 = _rand(rng, n2), _rand(rng, n1)
    idx = sorted(rng.choice(n1, 20, replace=False).tolist())
    for i in idx:
        d1[i] = at_distance(rng, d2[2], 30)
    a = np.zeros(n1, np.float32)
    for r in (1.0, 0.75):  # 1.0 accepts the lowest index, 0.75 rejects (second == best)
        cases.append(Case(f"tie_over16_r{r}", d1, a, d2, a[:n2].copy(), None, r, False, {"query": 2, "lowest": idx[0]}))
    # (c) ... with the listed ones claimed by earlier queries: the second is UNLISTED at exactly the last listed distance
    cases += _tie_beyond(seed + 2)
    # (d) every descriptor identical: every row full, the queries past the 16th fall back to the full-row scan; matched[i] = i
    rng = np.random.default_rng(seed + 3)
    n = 300
    d = np.repeat(_rand(rng, 1), n, 0)
    a = np.full(n, 77.0, np.float32)
    for r in (0.75, 0.3):
        cases.append(Case(f"all_identical_r{r}", d, a, d.copy(), a.copy(), None, r, True, {"identity": True}))
    return cases


def _tie_beyond(seed):
    """Query 16 has 17 candidates t_0 < .. < t_16 at distance D (the list of 16 is truncated at D); queries 0..15 claim t_0..t_15 first
    (8 bits from their own).  'full_row': D = 50, no other candidate: every listed one is claimed and the exact full-row scan finds t_16 at
    50 (second far): a match.  'ratio': an own best at 33 besides, D = 43, lowe_ratio 0.75: the unlisted t_16 is the second at 43 and
    0.75 * 43 < 33 rejects (a bound of 44 taken for the unlisted ones would accept)."""
    cases = []
    for variant, D, own in (("full_row", 50, None), ("ratio", 43, 33)):
        def make(rng, D=D, own=own, variant=variant):
            n1, n2 = 96, 17
            d2, d1 = _rand(rng, n2), _rand(rng, n1)
            tix = sorted(rng.choice(80, 17, replace=False).tolist())
            plants = {}
            for i in tix:
                d1[i] = at_distance(rng, d2[16], D)
                plants[(16, i)] = D
            for k in range(16):
                d2[k] = at_distance(rng, d1[tix[k]], 8)
                plants[(k, tix[k])] = 8
            if own is not None:
                d1[90] = at_distance(rng, d2[16], own)
                plants[(16, 90)] = own
            M = O.hamming_matrix(d1, d2).astype(int)
            if any(M[j, i] != dd for (j, i), dd in plants.items()):
                return None
            if any(np.delete(M[k], tix[k]).min() < 40 for k in range(16)):  # every claim is accepted at 0.75
                return None
            if np.delete(M[16], tix + ([90] if own is not None else [])).min() <= 70:
                return None
            a = np.zeros(n1, np.float32)
            return Case(f"tie_beyond_{variant}", d1, a, d2, a[:n2].copy(), None, 0.75, False, {"t": tix, "match16": own is None})
        cases.append(_retry(make, seed * 10 + len(cases)))
    return cases


# ---------------------------------------------------------------------------------------------------- 5. popcounts
def popcounts(seed=5):
    """all-zero, all-ones, one-bit, 255-bit and 126..129 / 254-bit descriptors on both sides (the int8 pieces of the MFMA popcount step at
    0 / 127 / 128 / 254 / 255 / 256), and all-zero queries against low-popcount targets."""
    rng = np.random.default_rng(seed)
    ones = np.full(32, 255, np.uint8)
    specials = [np.zeros(32, np.uint8), ones]
    for b in (0, 7, 8, 127, 128, 255):
        specials.append(from_bits([b]))    # popcount 1
        specials.append(flip(ones, [b]))   # popcount 255
    for k in (2, 126, 127, 128, 129, 254):
        specials.append(from_bits(_bits(rng, k)))
    sp = np.stack(specials)
    low = np.stack([from_bits(_bits(rng, k)) for k in (3, 5, 9, 20, 31, 40, 49, 50, 51, 60, 70)])
    high = np.stack([flip(ones, _bits(rng, k)) for k in (3, 9, 40, 50, 51)])
    d1 = np.concatenate([sp, low, high, _rand(rng, 30)])
    d2 = np.concatenate([sp[::-1], low[::2], high[::2], np.zeros((1, 32), np.uint8)])
    a1, a2 = np.full(len(d1), 45.0, np.float32), np.full(len(d2), 45.0, np.float32)
    cases = [Case(f"popcount_r{r}", d1, a1, d2, a2, None, r, False) for r in (0.75, 1.0, 0.5)]
    t = np.stack([from_bits(_bits(rng, k)) for k in list(range(1, 60, 3)) + [1, 2, 50, 51]])
    q = np.stack([np.zeros(32, np.uint8), from_bits([200]), np.zeros(32, np.uint8)])
    cases += [Case(f"popcount_zero_query_r{r}", t, np.zeros(len(t), np.float32), q, np.zeros(3, np.float32), None, r, False)
              for r in (0.75, 1.0)]
    return cases


# ---------------------------------------------------------------------------------------------------- 6. orientation gate
def _nx(x, to):
    return float(np.nextafter(F32(x), F32(to)))


# (query angle, target angle): the target is the query's nearest (10 bits); a fallback 30 bits away sits at the query's own angle, so the
# gate alone decides which one is matched
GATE_PAIRS = [
    # exactly 30 apart (kept) and the next float beyond (gated)
    (10.0, 40.0), (40.0, 10.0), (10.0, _nx(40.0, 99)), (_nx(40.0, 99), 10.0), (_nx(10.0, 0), 40.0), (10.0, _nx(40.0, 0)),
    # wrap-around at 0 / 360, -0.0
    (0.0, 330.0), (330.0, 0.0), (360.0, 30.0), (30.0, 360.0), (359.5, 0.25), (0.25, 359.5), (-0.0, 30.0), (-0.0, 330.0),
    (0.0, _nx(330.0, 0)), (360.0, _nx(30.0, 99)),
    # across bin edges at a difference of about 30: one-degree bins 31, 30 and 29 apart
    (_nx(1.0, 0), 31.0), (10.5, 40.5), (_nx(11.0, 0), 41.0), (40.99, 10.99), (_nx(360.0, 0), 29.999998), (0.5, 330.5), (359.0, 29.0),
    # outside [0, 360] on either side: no pruning, the gate still decides
    (-5.0, 20.0), (20.0, -5.0), (365.0, 30.0), (30.0, 365.0), (720.0, 10.0), (10.0, 720.0), (-30.0, 0.0),
    # non-finite
    (NAN, 10.0), (10.0, NAN), (float("inf"), 10.0), (10.0, float("-inf")),
    # query angles <= -500
    (-600.0, 10.0), (-600.0, -600.0), (-1000.0, -1000.0), (-500.0, -500.0), (-1000.0, 20.0),
]


def gate_kept(qa, ta) -> bool:
    return not (abs(O.angle_diff(float(F32(ta)), float(F32(qa)))) > 30.0)


def orientation(seed=6):
    cases = []
    for k, (qa, ta) in enumerate(GATE_PAIRS):
        def make(rng, qa=qa, ta=ta):
            n1, n2 = 40, 3
            d2, d1 = _rand(rng, n2), _rand(rng, n1)
            d1[23] = at_distance(rng, d2[1], 10)  # gate-deciding target
            d1[5] = at_distance(rng, d2[1], 30)   # fallback
            if not _verify(d1, d2, {(1, 23): 10, (1, 5): 30}, {1: 70, 0: 70, 2: 70}):
                return None
            a1 = _angles(rng, n1)
            a1[23] = F32(ta)
            a1[5] = F32(qa) if np.isfinite(qa) and 0 <= qa <= 360 else F32(0.0)
            a2 = np.full(n2, F32(qa), np.float32)  # every query at the same angle: the narrowest candidate window
            return d1, a1, d2, a2
        d1, a1, d2, a2 = _retry(make, seed * 100 + k)
        for check in (False, True):
            cases.append(Case(f"gate_{qa!r}_{ta!r}/ori{int(check)}", d1, a1, d2, a2, None, 0.75, check,
                              {"query": 1, "near": 23, "kept": (not check) or gate_kept(qa, ta)}))
    return cases


# ---------------------------------------------------------------------------------------------------- 7. claim chain
def domino(length, seed=7, valid2=None):
    """Query j's nearest target is t_{j-1} (10 bits), its second t_j (11 bits): t_j = t_{j-1} ^ D_j with 21-bit masks D_j disjoint from
    their neighbours, q_j = t_{j-1} ^ A_j with A_j a 10-bit subset of D_j, and q_0 = t_0 ^ A_0 (10 bits from t_0, 31 from t_1).  While
    t_{j-1} is free, 0.75 * 11 < 10 rejects q_j; once q_{j-1} has taken it, q_j takes t_j.  Sequentially matched[i] = i, and the replay
    needs one sweep per query."""
    def make(rng):
        n = length
        D, prev = [None], set()
        for j in range(1, n + 1):
            m = set(_bits(rng, 21, set(range(256)) - prev).tolist())
            D.append(m)
            prev = m
        t = np.empty((n, 32), np.uint8)
        t[0] = _rand(rng, 1)[0]
        for j in range(1, n):
            t[j] = flip(t[j - 1], sorted(D[j]))
        q = np.empty((n, 32), np.uint8)
        q[0] = flip(t[0], _bits(rng, 10, set(range(256)) - D[1]))
        for j in range(1, n):
            q[j] = flip(t[j - 1], _bits(rng, 10, D[j]))
        M = O.hamming_matrix(t, q).astype(int)
        idx = np.arange(n)
        if M[0, 0] != 10 or (M[idx[1:], idx[1:] - 1] != 10).any() or (M[idx[1:], idx[1:]] != 11).any():
            return None
        M[idx, idx] = 999
        M[idx[1:], idx[1:] - 1] = 999
        if M.min() < 20:
            return None
        a = np.zeros(n, np.float32)
        return Case(f"domino_{length}" + ("" if valid2 is None else "_head_masked"), t, a, q, a.copy(), valid2, 0.75, False, {"chain": True})
    return _retry(make, seed)


# ---------------------------------------------------------------------------------------------------- 8. valid2
def valid2_masks(seed=8):
    rng = np.random.default_rng(seed)
    n1, n2 = 300, 260
    d1 = _rand(rng, n1)
    src = rng.integers(0, n1 // 3, n2)  # several queries per target: contested claims
    d2 = np.stack([at_distance(rng, d1[s], int(rng.integers(0, 30))) for s in src])
    a1 = _angles(rng, n1)
    a2 = ((a1[src] + rng.normal(0, 10, n2)) % 360).astype(np.float32)
    base = Case("valid2_none", d1, a1, d2, a2, None, 0.8, True)
    exp = base.oracle()
    claimers = np.zeros(n2, np.uint8)
    claimers[exp[exp >= 0]] = 1  # the queries that take a target when all are live
    cases = [base,
             dataclasses.replace(base, name="valid2_ones", valid2=np.ones(n2, np.uint8)),
             dataclasses.replace(base, name="valid2_zero", valid2=np.zeros(n2, np.uint8)),
             dataclasses.replace(base, name="valid2_alternating", valid2=(np.arange(n2) % 2).astype(np.uint8)),
             dataclasses.replace(base, name="valid2_no_claimers", valid2=(1 - claimers).astype(np.uint8), info={"claimers": claimers})]
    head = np.ones(200, np.uint8)
    head[0] = 0
    cases.append(domino(200, seed=seed, valid2=head))  # the chain's head masked: nobody can ever take anything
    return cases


def all_classes(big: bool = False) -> dict:
    """class name -> cases.  big adds the long claim chains (1 000 and 2 560 queries: as many replay sweeps)."""
    return {
        "threshold": [threshold(check=True), threshold(seed=11, check=False)],
        "ratio_equality": ratio_equality(),
        "around_dmax": around_dmax(),
        "ties": ties(),
        "popcount": popcounts(),
        "orientation": orientation(),
        "domino": [domino(300)] + ([domino(1000, seed=71), domino(2560, seed=72)] if big else []),
        "valid2": valid2_masks(),
    }
