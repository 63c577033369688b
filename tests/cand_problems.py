"""Planted problems for the CSR candidate matcher (svgpu_match_candidates: k_cand_dist + k_cand_replay_lds / k_cand_replay / k_area_replay),
the matcher behind projection::*, fuse, bow_tree::*, robust::match_for_triangulation and area::match_in_consistent_area.

Everything here is integer: a target descriptor is a query descriptor with exactly d bits flipped, so every distance of every candidate
list is set by hand and the decisions land exactly on the matcher's boundaries -- best == thr, lowe_ratio * second == best in fp32, the
same-octave exception, the pruning of useless seconds, ties at the seams of the three sort implementations, every gate, lists longer than
the staged head of the LDS replay, claim chains across the 1 024-query chunks, AREA's take-over.  numpy + the CPU oracle only.

  Builder                 queries with lists of (target, distance) -> descriptors (a forest of "flip d bits" edges), verified with
                          O.hamming_matrix
  py_match_candidates     literal restatement of the reference loops (match/projection.cc:13-207, match/bow_tree.cc:66-140, :200-237,
                          match/area.cc:8-98), with deliberately wrong variants for the sensitivity tests
  embed                   pads a case with empty-list queries and unreferenced targets so that it reaches a chosen replay form
  replay_form / find_forms   svgpu_selftest_cand_replay_form and the paddings (nq, nt) that give each form
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from oracle import oracle as O

F32 = np.float32
NAN = float("nan")
BEST_ONLY, RATIO_SAME_OCTAVE, RATIO, TRIANGULATION, AREA = 0, 1, 2, 3, 4
MAX_HAMMING_DIST = 256
CHUNK = 1024  # queries per chunk of k_cand_replay_lds


@dataclasses.dataclass
class Case:
    name: str
    mode: int
    thr: int
    ratio: float
    check: bool
    qdesc: np.ndarray
    tdesc: np.ndarray
    cand_off: np.ndarray
    cand_idx: np.ndarray
    cand_skip: np.ndarray | None = None
    t_octave: np.ndarray | None = None
    q_valid: np.ndarray | None = None
    occupied: np.ndarray | None = None
    q_angle: np.ndarray | None = None
    t_angle: np.ndarray | None = None
    q_xright: np.ndarray | None = None
    t_xright: np.ndarray | None = None
    q_xr_tol: np.ndarray | None = None
    expect: np.ndarray | None = None   # designed answer per query (target index, -1, or -9 = not designed by hand)
    planted: np.ndarray | None = None  # designed distance per CSR entry
    info: dict = dataclasses.field(default_factory=dict)

    @property
    def nq(self):
        return len(self.qdesc)

    @property
    def nt(self):
        return len(self.tdesc)

    def kwargs(self):
        """the optional arrays, by the names both O.match_candidates and match.projection.match_candidates use"""
        names = ("cand_skip", "t_octave", "q_valid", "occupied", "q_angle", "t_angle", "q_xright", "t_xright", "q_xr_tol")
        return {n: getattr(self, n) for n in names if getattr(self, n) is not None}

    def oracle(self):
        return O.match_candidates(self.qdesc, self.tdesc, self.cand_off, self.cand_idx, check_orientation=self.check, thr=self.thr,
                                  lowe_ratio=self.ratio, mode=self.mode, **self.kwargs())


# ---------------------------------------------------------------------------------------------------- bits
def flip(desc, bits):
    out = desc.copy()
    for b in np.asarray(bits, int):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def at_distance(rng, desc, k):
    """a descriptor exactly k bits away from `desc`"""
    return flip(desc, rng.choice(256, k, replace=False))


def far(rng):
    """an unrelated target: farther than every threshold in use"""
    return int(rng.integers(104, 150))


def entry_distances(c: Case) -> np.ndarray:
    """Hamming distance of every CSR entry"""
    if len(c.cand_idx) == 0:
        return np.zeros(0, int)
    qrep = np.repeat(np.arange(c.nq), np.diff(c.cand_off))
    return np.unpackbits(c.qdesc[qrep] ^ c.tdesc[c.cand_idx], axis=1).sum(1).astype(int)


class Builder:
    """Collects queries with hand-made candidate lists.  An entry is (target, distance[, skip]); the (query, target, distance) edges must
    form a forest, so that descriptors follow by flipping `distance` random bits along every edge."""

    def __init__(self, seed, additive=None):
        self.rng = np.random.default_rng(seed)
        self.additive = additive  # (a per query, b per target): distance(q, t) = a[q] + b[t] for EVERY pair, where a forest will not do
        self.t = []  # dicts octave, occupied, angle, xright
        self.q = []  # dicts entries, valid, angle, xright, tol, expect

    def target(self, octave=0, occupied=0, angle=0.0, xright=-1.0):
        self.t.append(dict(octave=octave, occupied=occupied, angle=angle, xright=xright))
        return len(self.t) - 1

    def fars(self, n, **kw):
        """n entries on fresh unrelated targets"""
        return [(self.target(**kw), far(self.rng)) for _ in range(n)]

    def query(self, entries, expect=-9, valid=1, angle=0.0, xright=0.0, tol=0.0):
        self.q.append(dict(entries=[(e[0], e[1], e[2] if len(e) > 2 else 0) for e in entries], valid=valid, angle=angle, xright=xright,
                           tol=tol, expect=expect))
        return len(self.q) - 1

    def _descriptors(self, rng):
        nq, nt = len(self.q), len(self.t)
        adj = {}
        for qi, q in enumerate(self.q):
            for t, d, _ in q["entries"]:
                adj.setdefault(("q", qi), []).append((("t", t), d))
                adj.setdefault(("t", t), []).append((("q", qi), d))
        if self.additive is not None:  # one base descriptor; queries differ from it in the low 128 bits, targets in the high 128
            a, b = self.additive
            base = rng.integers(0, 256, 32, dtype=np.uint8)
            return (np.stack([flip(base, rng.choice(128, k, replace=False)) for k in a]),
                    np.stack([flip(base, 128 + rng.choice(128, k, replace=False)) for k in b]))
        desc = {}
        for root in [("q", i) for i in range(nq)] + [("t", i) for i in range(nt)]:
            if root in desc:
                continue
            desc[root] = rng.integers(0, 256, 32, dtype=np.uint8)
            stack = [root]
            while stack:
                a = stack.pop()
                for b, d in adj.get(a, ()):
                    if b not in desc:
                        desc[b] = at_distance(rng, desc[a], d)
                        stack.append(b)
        return np.stack([desc[("q", i)] for i in range(nq)]), np.stack([desc[("t", i)] for i in range(nt)])

    def build(self, name, mode, thr, ratio, check=False, stereo=False, **info) -> Case:
        nq = len(self.q)
        off = np.zeros(nq + 1, np.int32)
        off[1:] = np.cumsum([len(q["entries"]) for q in self.q])
        ent = [e for q in self.q for e in q["entries"]]
        idx = np.array([e[0] for e in ent], np.int32)
        planted = np.array([e[1] for e in ent], int)
        skip = np.array([e[2] for e in ent], np.uint8)
        c = None
        for _ in range(20):
            qd, td = self._descriptors(self.rng)
            c = Case(name, mode, thr, float(ratio), bool(check), qd, td, off, idx, planted=planted, info=info)
            D = O.hamming_matrix(td, qd).astype(int)  # [query, target]
            if np.array_equal(D[np.repeat(np.arange(nq), np.diff(off)), idx], planted):
                break
        else:
            raise RuntimeError(f"{name}: the (query, target, distance) edges are not a forest")
        c.expect = np.array([q["expect"] for q in self.q], np.int32)
        c.t_octave = np.array([t["octave"] for t in self.t], np.int32)
        if skip.any():
            c.cand_skip = skip
        if any(not q["valid"] for q in self.q):
            c.q_valid = np.array([q["valid"] for q in self.q], np.uint8)
        if any(t["occupied"] for t in self.t):
            c.occupied = np.array([t["occupied"] for t in self.t], np.uint8)
        if check or mode == AREA:
            c.q_angle = np.array([q["angle"] for q in self.q], np.float32)
            c.t_angle = np.array([t["angle"] for t in self.t], np.float32)
        if stereo:
            c.q_xright = np.array([q["xright"] for q in self.q], np.float32)
            c.t_xright = np.array([t["xright"] for t in self.t], np.float32)
            c.q_xr_tol = np.array([q["tol"] for q in self.q], np.float32)
        return c


# ---------------------------------------------------------------------------------------------------- the restatement
def py_angle_diff(a1, a2):
    """util/angle.cc:7-16: float difference, double constants"""
    with np.errstate(invalid="ignore"):
        ret = F32(a1) - F32(a2)
        if float(ret) <= -180.0:
            ret = F32(float(ret) + 360.0)
        if float(ret) > 180.0:
            ret = F32(float(ret) - 360.0)
    return ret


WRONG = ("thr_le", "tri_start_256", "ratio_le", "ignore_levels", "prune_thr_only", "later_tie", "tri_sorted", "head_stop", "chunk_blind",
         "area_le", "gate30_ge", "xright_ge0", "tol_le")


def _gated(c, q, pos, wrong):
    """the per-candidate gates that do not depend on earlier queries: projection.cc:56-62, :176-185, bow_tree.cc:83-85, cand_skip"""
    t = int(c.cand_idx[pos])
    if c.cand_skip is not None and c.cand_skip[pos]:
        return True
    if c.mode != AREA and c.t_xright is not None:
        tx = F32(c.t_xright[t])
        if (F32(0) <= tx) if "xright_ge0" in wrong else (F32(0) < tx):
            err = np.abs(F32(c.q_xright[q]) - tx)
            tol = F32(c.q_xr_tol[q])
            if (tol <= err) if "tol_le" in wrong else (tol < err):
                return True
    if c.check:
        a = float(np.abs(py_angle_diff(c.q_angle[q], c.t_angle[t])))
        if (a >= 30.0) if "gate30_ge" in wrong else (a > 30.0):
            return True
    return False


def _decide(c, q, dist, taken, wrong=(), K=None):
    """One query of the modes BEST_ONLY .. TRIANGULATION: scan the list in order, `taken(t)` = the keypoint already holds a landmark or was
    given to an earlier query.  Returns the target or -1."""
    lo, hi = int(c.cand_off[q]), int(c.cand_off[q + 1])
    if lo == hi:
        return -1
    mode, thr, ratio = c.mode, c.thr, F32(c.ratio)
    lvl = (lambda t: int(c.t_octave[t])) if c.t_octave is not None else (lambda t: 0)
    tri = mode == TRIANGULATION
    live = []  # (position, target, distance) of the entries that pass the gates, in scan order
    for pos in range(lo, hi):
        t = int(c.cand_idx[pos])
        if taken(t) or _gated(c, q, pos, wrong):
            continue
        live.append((pos, t, int(dist[pos])))
    if "prune_thr_only" in wrong and mode == RATIO_SAME_OCTAVE:
        live = [e for e in live if not thr < e[2]]
    if "head_stop" in wrong and not tri:  # a sorted walk that gives up after K entries, taken ones included
        every = [(pos, int(c.cand_idx[pos]), int(dist[pos])) for pos in range(lo, hi)
                 if not _gated(c, q, pos, wrong) and not (c.occupied is not None and c.occupied[int(c.cand_idx[pos])])]
        head = sorted(every, key=lambda e: (e[2], e[0]))[:K]
        live = [e for e in head if not taken(e[1])]
    if "tri_sorted" in wrong and tri:  # first two of the (distance, position) order
        live = sorted([e for e in live if e[2] <= thr], key=lambda e: (e[2], e[0]))[:2]
        best, best_idx = (live[0][2], live[0][1]) if live and live[0][2] < thr else (thr, -1)
        second = live[1][2] if len(live) > 1 and best_idx >= 0 else MAX_HAMMING_DIST
        if best_idx < 0:
            return -1
        return -1 if ratio * F32(second) < F32(best) else best_idx
    best = (MAX_HAMMING_DIST if "tri_start_256" in wrong else thr) if tri else MAX_HAMMING_DIST
    second = MAX_HAMMING_DIST
    best_lvl = second_lvl = best_idx = -1
    for pos, t, d in live:
        if tri and (thr < d or best < d):
            continue
        if (d <= best and "later_tie" in wrong and not (tri and best_idx < 0 and d == best)) or d < best:
            second, second_lvl = best, best_lvl
            best, best_lvl, best_idx = d, lvl(t), t
        elif d < second:
            second, second_lvl = d, lvl(t)
    if mode == RATIO_SAME_OCTAVE:
        if (best < thr) if "thr_le" in wrong else (best <= thr):
            same = True if "ignore_levels" in wrong else best_lvl == second_lvl
            fails = (F32(best) >= ratio * F32(second)) if "ratio_le" in wrong else (F32(best) > ratio * F32(second))
            if same and fails:
                return -1
            return best_idx
        return -1
    if (thr <= best) if "thr_le" in wrong and not tri else (thr < best):
        return -1
    if mode == BEST_ONLY:
        return best_idx
    if best_idx < 0:
        return -1
    if (ratio * F32(second) <= F32(best)) if "ratio_le" in wrong else (ratio * F32(second) < F32(best)):
        return -1
    return best_idx


def py_match_candidates(c: Case, wrong=(), K=None) -> np.ndarray:
    """The reference loops, literally: queries in index order, each scans its list in order.  `wrong` names deliberate mistakes."""
    wrong = (wrong,) if isinstance(wrong, str) else tuple(wrong)
    assert all(w in WRONG for w in wrong)
    dist = entry_distances(c)
    out = np.full(c.nq, -1, np.int32)
    if c.mode == AREA:  # area.cc:8-98
        mdist = {}
        holder = {}
        ratio = F32(c.ratio)
        for q in range(c.nq):
            if c.q_valid is not None and not c.q_valid[q]:
                continue
            best = second = MAX_HAMMING_DIST
            best_idx = -1
            for pos in range(int(c.cand_off[q]), int(c.cand_off[q + 1])):
                t = int(c.cand_idx[pos])
                if _gated(c, q, pos, wrong):
                    continue
                d = int(dist[pos])
                held = mdist.get(t, MAX_HAMMING_DIST)
                if (held < d) if "area_le" in wrong else (held <= d):
                    continue
                if d < best:
                    second, best, best_idx = best, d, t
                elif d < second:
                    second = d
            if (c.thr <= best) if "thr_le" in wrong else (c.thr < best):
                continue
            if best_idx < 0:
                continue
            if (F32(second) * ratio <= F32(best)) if "ratio_le" in wrong else (F32(second) * ratio < F32(best)):
                continue
            if best_idx in holder:
                out[holder[best_idx]] = -1
            out[q] = best_idx
            holder[best_idx] = q
            mdist[best_idx] = best
        return out
    claimed = {}  # target -> the query that took it
    for q in range(c.nq):
        if c.q_valid is not None and not c.q_valid[q]:
            continue

        def taken(t):
            if c.occupied is not None and c.occupied[t]:
                return True
            if t not in claimed:
                return False
            return not ("chunk_blind" in wrong and q >= CHUNK and claimed[t] < CHUNK)
        m = _decide(c, q, dist, taken, wrong, K)
        out[q] = m
        if m >= 0 and m not in claimed:
            claimed[m] = q
    return out


def py_fixed_point(c: Case):
    """The replay as the kernels run it (modes 0 - 3): every query decides against the owner table of the previous sweep, the winners claim
    (owner = the earliest claimant), until nothing changes.  Returns (matches, number of sweeps that changed something)."""
    dist = entry_distances(c)
    active = [q for q in range(c.nq) if c.cand_off[q + 1] > c.cand_off[q] and (c.q_valid is None or c.q_valid[q])]
    match = {q: -2 for q in active}
    owner = {}
    sweeps = 0
    while True:
        new = {}
        for q in active:
            new[q] = _decide(c, q, dist, lambda t: bool(c.occupied is not None and c.occupied[t]) or owner.get(t, 1 << 30) < q)
        if new == match:
            break
        match = new
        sweeps += 1
        owner = {}
        for q in active:
            if match[q] >= 0:
                owner[match[q]] = min(owner.get(match[q], 1 << 30), q)
    out = np.full(c.nq, -1, np.int32)
    for q in active:
        out[q] = match[q]
    return out, sweeps


# ---------------------------------------------------------------------------------------------------- forms and embedding
def replay_form(nq, nt, mode, with_cnt=0):
    """svgpu_selftest_cand_replay_form: K >= 0 / -1 = global for the modes 0 - 3; 1 = LDS / 0 = global state for AREA"""
    from stella_vslam_amd import _lib
    return int(_lib.lib().svgpu_selftest_cand_replay_form(int(nq), int(nt), int(with_cnt), int(mode)))


def py_replay_form(nq, nt, mode, with_cnt=0):
    """the same choice restated from the launch code's formula (150 KiB budget, at most 64 staged entries; AREA: 60 KiB of state)"""
    if mode == AREA:
        return 1 if (2 * nt + nq) * 4 <= 60 * 1024 else 0
    r4 = lambda n: (n + 3) & ~3
    tables = (nt + nq + nq + 1 + (nq if with_cnt else 0)) * 4 + 2 * r4(nt) + r4(nq) + 16
    if tables > 150 * 1024:
        return -1
    return min(64, (150 * 1024 - tables) // (nq * 4)) if nq > 0 else 0


NQ_TWO_CHUNKS = 1200  # more than one chunk of 1 024 queries
FORM_START = {"K5": 19500, "K4": 20000, "K3": 21000, "K1": 22500, "K0": 23000, "global": 24000}  # where the search for nt starts
FORM_WANT = {"K5": 5, "K4": 4, "K3": 3, "K1": 1, "K0": 0, "global": -1}


@functools.lru_cache(maxsize=None)
def find_forms(form_of=replay_form):
    """name -> (nq, nt, expected form) for the modes 0 - 3, and "area_lds" / "area_global" for AREA.  The sizes are SEARCHED with the
    library's own form function, never assumed.  64 staged entries per list need 256 bytes per query, so that form cannot hold two chunks of
    queries (1 025 x 256 B exceed the budget): it runs with 500 queries, and "Kmax" is the largest K that two chunks allow."""
    forms = {}
    nq, nt = 500, 3000
    assert form_of(nq, nt, RATIO) == 64
    forms["K64"] = (nq, nt, 64)
    forms["Kmax"] = (NQ_TWO_CHUNKS, 3000, form_of(NQ_TWO_CHUNKS, 3000, RATIO))
    assert 5 < forms["Kmax"][2] < 64
    for name, start in FORM_START.items():
        for nt in list(range(start, 26000, 4)) + list(range(start, 3000, -4)):
            if form_of(NQ_TWO_CHUNKS, nt, RATIO) == FORM_WANT[name]:
                forms[name] = (NQ_TWO_CHUNKS, nt, FORM_WANT[name])
                break
        else:
            raise RuntimeError(f"no table size gives the form {name}")
    forms["area_lds"] = (NQ_TWO_CHUNKS, 3000, 1)
    forms["area_global"] = (2000, 7000, 0)
    for name in ("area_lds", "area_global"):
        assert form_of(*forms[name][:2], AREA) == forms[name][2], name
    return forms


def forms_of(mode):
    return ("area_lds", "area_global") if mode == AREA else ("K64", "Kmax", "K5", "K4", "K3", "K1", "K0", "global")


@functools.lru_cache(maxsize=None)
def _padding(nq_total, nt_total):
    rng = np.random.default_rng(nq_total * 100003 + nt_total)
    return rng.integers(0, 256, (nq_total, 32), dtype=np.uint8), rng.integers(0, 256, (nt_total, 32), dtype=np.uint8)


def embed(c: Case, nq_total, nt_total, q_at=None, t_at=None):
    """The case inside tables of nq_total queries and nt_total targets: query i moves to q_at[i] (increasing: the serial order is kept),
    target k to t_at[k]; the other queries have empty lists, the other targets are listed nowhere.  Defaults: the queries as a block that
    straddles index 1 024 (or where c.info["q_at"] / c.info["q_start"] puts them, when the table is long enough), the targets scattered over
    the whole table.  Returns (embedded case, expected answer = the padded answer of the original)."""
    assert c.nq <= nq_total and c.nt <= nt_total
    if q_at is None:
        q_at = c.info.get("q_at")
        if q_at is None or max(q_at) >= nq_total:
            start = min(c.info.get("q_start", max(0, CHUNK - c.nq // 2)), nq_total - c.nq)
            q_at = start + np.arange(c.nq)
    q_at = np.asarray(q_at, int)
    assert len(q_at) == c.nq and (np.diff(q_at) > 0).all() and q_at[-1] < nq_total
    if t_at is None:
        t_at = np.random.default_rng(c.nt * 7919 + nt_total).permutation(nt_total)[:c.nt]
    t_at = np.asarray(t_at, int)
    assert len(t_at) == c.nt and len(set(t_at.tolist())) == c.nt
    qd, td = (a.copy() for a in _padding(nq_total, nt_total))
    qd[q_at], td[t_at] = c.qdesc, c.tdesc
    cnt = np.zeros(nq_total, np.int64)
    cnt[q_at] = np.diff(c.cand_off)
    off = np.zeros(nq_total + 1, np.int32)
    off[1:] = np.cumsum(cnt)

    def pad(a, n, at, fill, dtype):
        if a is None:
            return None
        out = np.full(n, fill, dtype)
        out[at] = a
        return out
    e = Case(c.name, c.mode, c.thr, c.ratio, c.check, qd, td, off, t_at[c.cand_idx].astype(np.int32), cand_skip=c.cand_skip,
             t_octave=pad(c.t_octave, nt_total, t_at, 0, np.int32), q_valid=pad(c.q_valid, nq_total, q_at, 1, np.uint8),
             occupied=pad(c.occupied, nt_total, t_at, 0, np.uint8), q_angle=pad(c.q_angle, nq_total, q_at, 0, np.float32),
             t_angle=pad(c.t_angle, nt_total, t_at, 0, np.float32), q_xright=pad(c.q_xright, nq_total, q_at, 0, np.float32),
             t_xright=pad(c.t_xright, nt_total, t_at, -1, np.float32), q_xr_tol=pad(c.q_xr_tol, nq_total, q_at, 0, np.float32),
             planted=c.planted, info=dict(c.info, q_at=q_at, t_at=t_at))
    return e, q_at, t_at


def embedded_answer(answer, q_at, t_at, nq_total):
    out = np.full(nq_total, -1, np.int32)
    a = np.asarray(answer)
    out[q_at] = np.where(a >= 0, t_at[np.maximum(a, 0)], -1)
    return out


# ---------------------------------------------------------------------------------------------------- 1. threshold
MODE_NAMES = {BEST_ONLY: "best_only", RATIO_SAME_OCTAVE: "same_octave", RATIO: "ratio", TRIANGULATION: "triangulation", AREA: "area"}


def threshold():
    """best = thr - 1, thr, thr + 1, alone in its list and with an unrelated second; lowe_ratio 1 keeps the ratio test out of the way
    (TRIANGULATION's second starts at thr).  TRIANGULATION's running best starts AT thr, so best == thr never becomes a best."""
    cases = []
    for thr in (50, 100):
        for mode in range(5):
            B = Builder(100 + thr + mode)
            for with_far in (False, True):
                for best in (thr - 1, thr, thr + 1):
                    t = B.target()
                    ok = best < thr or (best == thr and mode != TRIANGULATION)
                    B.query([(t, best)] + (B.fars(1) if with_far else []), expect=t if ok else -1)
            cases.append(B.build(f"threshold/{MODE_NAMES[mode]}/thr{thr}", mode, thr, 1.0))
    return cases


# ---------------------------------------------------------------------------------------------------- 2. ratio equality
def accepts(best, second, ratio):
    """rejected iff lowe_ratio * second < best, in fp32"""
    return not (F32(ratio) * F32(second) < F32(best))


RATIO_TRIPLES = {0.75: [(60, 80), (45, 60), (48, 64), (30, 40)], 0.5: [(50, 100), (25, 50), (33, 66)], 0.625: [(30, 48), (50, 80)],
                 # 0.7f * 100 is 69.9999988 exactly and 70 after the fp32 rounding of the product: accepted in fp32, rejected in double
                 0.7: [(70, 100), (35, 50), (63, 90)], 0.8: [(60, 75), (48, 60), (40, 50)]}


def ratio_equality():
    """(best, second) with lowe_ratio * second == best in fp32, and second one step to either side; both list orders (TRIANGULATION gets
    its second as a superseded best, so second comes first there)"""
    cases = []
    for ratio, triples in RATIO_TRIPLES.items():
        for mode in (RATIO_SAME_OCTAVE, RATIO, TRIANGULATION, AREA):
            thr = 50 if mode == AREA else 100
            B = Builder(int(ratio * 1000) + mode)
            for best, second_eq in triples:
                if best > thr:
                    continue
                assert F32(ratio) * F32(second_eq) == F32(best)
                for second in (second_eq - 1, second_eq, second_eq + 1):
                    for second_first in ((True,) if mode == TRIANGULATION else (False, True)):
                        tb, ts = B.target(), B.target()
                        ent = [(ts, second), (tb, best)] if second_first else [(tb, best), (ts, second)]
                        B.query(ent, expect=tb if accepts(best, second, ratio) else -1)
            cases.append(B.build(f"ratio_equality/{MODE_NAMES[mode]}/r{ratio}", mode, thr, ratio))
    return cases


# ---------------------------------------------------------------------------------------------------- 3. same octave, pruning, best only
def same_octave():
    thr, ratio = 100, 0.8
    B = Builder(31)
    tb, ts = B.target(octave=2), B.target(octave=2)
    B.query([(tb, 60), (ts, 70)], expect=-1)                       # same octave, 60 > 0.8 * 70: rejected
    tb, ts = B.target(octave=2), B.target(octave=3)
    B.query([(tb, 60), (ts, 70)], expect=tb)                       # the same pair in different octaves
    tb, ts = B.target(octave=3), B.target(octave=2)
    B.query([(ts, 70), (tb, 60)], expect=tb)
    tb, ts = B.target(octave=0), B.target(octave=0)
    B.query([(tb, 60), (ts, 76)], expect=tb)                       # same octave, ratio passes (60.8)
    tb = B.target(octave=0)
    B.query([(tb, 60)], expect=tb)                                 # no second at all: its level stays -1
    tb, ts = B.target(octave=2), B.target(octave=2, occupied=1)
    B.query([(tb, 60), (ts, 70)], expect=tb)                       # the only second is occupied
    tb, ts = B.target(octave=2), B.target(octave=2)
    B.query([(tb, 60), (ts, 70, 1)], expect=tb)                    # ... or dropped by the caller
    # seconds around the pruning boundary of k_cand_dist (thr < d, and lowe_ratio * d just below / equal to / above thr)
    for second, ok in ((124, False), (125, True), (126, True)):
        for best in (100, 99):
            passes = not (F32(best) > F32(ratio) * F32(second))
            assert best != 100 or passes == ok
            tb, ts = B.target(octave=1), B.target(octave=1)
            B.query([(ts, second), (tb, best), (B.target(octave=1), 140), (B.target(octave=1), 150)], expect=tb if passes else -1)
            tb, ts, tx = B.target(octave=1), B.target(octave=1), B.target(octave=1)
            B.query([(tb, best), (tx, second + 4), (ts, second)], expect=tb if passes else -1)
    tb, ts = B.target(octave=1), B.target(octave=1)
    B.query([(tb, 101), (ts, 102)], expect=-1)                     # best just over thr
    cases = [B.build("same_octave/levels_and_pruning", RATIO_SAME_OCTAVE, thr, ratio)]
    B = Builder(32)
    for best, second in ((40, 41), (40, 45), (100, 101), (100, 100), (101, 120), (99, 230)):
        tb, ts = B.target(), B.target()
        B.query([(ts, second), (tb, best)] if best % 2 else [(tb, best), (ts, second)], expect=tb if best <= thr else -1)
    cases.append(B.build("same_octave/best_only_with_second", BEST_ONLY, thr, ratio))
    return cases


# ---------------------------------------------------------------------------------------------------- 4. triangulation order
def triangulation_order():
    """Lists whose outcome under "skip anything farther than the running best; second = the last superseded best" differs from the first
    two entries of the sorted order: ascending distances leave second at thr, descending ones make the previous best the second."""
    thr, ratio = 100, 0.8
    B = Builder(41)
    patterns = {"ascending": ([70, 80, 90], True), "descending": ([90, 80, 70], False), "dip": ([80, 70, 75], False),
                "rise": ([70, 75, 80], True), "equal": ([70, 70, 90], False), "late_best": ([100, 88, 71], False)}
    for L in (3, 64, 65, 1025):
        for name, (ds, ok) in patterns.items():
            if L == 1025 and name not in ("ascending", "descending"):
                continue
            pos = {0: ds[0], L // 2: ds[1], L - 1: ds[2]}
            ent, tbest = [], None
            for p in range(L):
                if p in pos:
                    t = B.target()
                    ent.append((t, pos[p]))
                    if pos[p] == min(ds) and tbest is None:
                        tbest = t
                else:
                    ent += B.fars(1)
            B.query(ent, expect=tbest if ok else -1)
    return [B.build("triangulation_order/lengths_3_64_65_1025", TRIANGULATION, thr, ratio)]


# ---------------------------------------------------------------------------------------------------- 5. ties
TIE_POSITIONS = ((0, 1), (62, 63), (63, 64), (64, 65), (1022, 1023), (1023, 1024))


def ties():
    """Equal best distances at the seams of the sort implementations (64 lanes of the register network, the LDS network up to 1 024, the
    unsorted walk beyond): the earlier scan position wins.  The rest of a list is far or gated."""
    cases = []
    for mode, ratio in ((BEST_ONLY, 0.8), (RATIO, 1.0)):
        B = Builder(50 + mode)
        for a, b in TIE_POSITIONS:
            ent, first = [], None
            for p in range(b + 1):
                if p in (a, b):
                    t = B.target()
                    ent.append((t, 40))
                    first = t if first is None else first
                elif p % 3 == 0:
                    ent.append((B.target(), 30, 1))  # closer, but dropped by the caller
                else:
                    ent += B.fars(1)
            B.query(ent, expect=first)
        t = B.target()
        B.query([(t, 40), (t, 40)], expect=t)  # the same target twice in one list
        cases.append(B.build(f"ties/positions/{MODE_NAMES[mode]}", mode, 100, ratio))
    B = Builder(53)
    for oct_b, oct_s, mode_ok in ((0, 0, False), (0, 1, True)):
        tb, ts = B.target(octave=oct_b), B.target(octave=oct_s)
        B.query([(tb, 40), (ts, 40)], expect=tb if mode_ok else -1)
    t = B.target()
    B.query([(t, 40), (t, 40)], expect=-1)
    cases.append(B.build("ties/best_equals_second/same_octave", RATIO_SAME_OCTAVE, 100, 0.9))
    for mode in (RATIO, TRIANGULATION, AREA):
        B = Builder(54 + mode)
        tb, ts = B.target(), B.target()
        B.query([(tb, 40), (ts, 40)], expect=-1)  # second == best: rejected whenever lowe_ratio < 1
        t = B.target()
        B.query([(t, 40), (t, 40)], expect=-1)    # ... also when the second is the same target again
        tb = B.target()
        B.query([(tb, 40)] + B.fars(3), expect=tb)  # (TRIANGULATION: second = thr = 50, and 0.9 * 50 < 40 is false)
        cases.append(B.build(f"ties/best_equals_second/{MODE_NAMES[mode]}", mode, 50, 0.9))
    return cases


# ---------------------------------------------------------------------------------------------------- 6. gates
def _next(x, towards):
    return float(np.nextafter(F32(x), F32(towards)))


def gate_specs(area=False):
    """(name, query attributes, target attributes, entry skip, gated?)"""
    specs = [("skip", {}, {}, 1, True),
             ("angle+30", dict(angle=30.0), dict(angle=0.0), 0, False),
             ("angle+30.000002", dict(angle=_next(30, 40)), dict(angle=0.0), 0, True),
             ("angle-30", dict(angle=330.0), dict(angle=0.0), 0, False),
             ("angle-30.00003", dict(angle=_next(330, 0)), dict(angle=0.0), 0, True),
             ("angle-180", dict(angle=0.0), dict(angle=180.0), 0, True),
             ("angle+180", dict(angle=180.0), dict(angle=0.0), 0, True),
             ("angle-179.99998", dict(angle=0.0), dict(angle=_next(180, 0)), 0, True),
             ("angle+350", dict(angle=355.0), dict(angle=5.0), 0, False),
             ("angle_nan_q", dict(angle=NAN), dict(angle=10.0), 0, False),
             ("angle_nan_t", dict(angle=10.0), dict(angle=NAN), 0, False)]
    if not area:
        st = dict(xright=10.0, tol=2.0)
        specs += [("occupied", {}, dict(occupied=1), 0, True),
                  ("xright_err3", st, dict(xright=13.0), 0, True),
                  ("xright_err==tol", st, dict(xright=12.0), 0, False),
                  ("xright_tol_one_ulp_less", dict(xright=10.0, tol=_next(2, 0)), dict(xright=12.0), 0, True),
                  ("xright-1", st, dict(xright=-1.0), 0, False),
                  ("xright0", st, dict(xright=0.0), 0, False),
                  ("xright_denormal", st, dict(xright=float(np.nextafter(F32(0), F32(1)))), 0, True),
                  ("xright_far_but_negative", st, dict(xright=-50.0), 0, False)]
    return specs


def gates():
    """The would-be best, or the would-be second, removed by each gate in turn -- and kept on the other side of the gate's boundary"""
    cases = []
    for mode in range(5):
        area = mode == AREA
        B = Builder(60 + mode)
        hand = mode in (RATIO, AREA)  # the modes the expectations below are written for
        for name, qa, ta, skip, gated in gate_specs(area):
            tx, to = B.target(**ta), B.target(angle=qa.get("angle", 0.0) if not np.isnan(qa.get("angle", 0.0)) else 0.0)
            B.query([(tx, 30, skip), (to, 45)], expect=(to if gated else tx) if hand else -9, **qa)      # 0.8 * 45 = 36: 30 passes
            tb, tx = B.target(angle=qa.get("angle", 0.0) if not np.isnan(qa.get("angle", 0.0)) else 0.0), B.target(**ta)
            B.query([(tb, 40), (tx, 44, skip)], expect=(tb if gated else -1) if hand else -9, **qa)      # 0.8 * 44 = 35.2 < 40
        # a list whose entries are all gated
        ent = [(B.target(), 20, 1), (B.target(angle=90.0), 25)]
        if not area:
            ent += [(B.target(occupied=1), 22), (B.target(xright=20.0), 24)]
        B.query(ent, expect=-1, xright=10.0, tol=2.0)
        # live entries behind 64 gated ones
        for tail in ((40,), (40, 44), (44, 40)):
            ent = [(B.target(), 10 + p % 20, 1) if (area or p % 2) else (B.target(occupied=1), 10 + p % 20) for p in range(64)]
            tt = [B.target() for _ in tail]
            ent += list(zip(tt, tail))
            B.query(ent, expect=(tt[tail.index(40)] if len(tail) == 1 else -1) if hand else -9)
        cases.append(B.build(f"gates/{MODE_NAMES[mode]}", mode, 50 if area else 100, 0.8, check=True, stereo=not area))
    return cases


# ---------------------------------------------------------------------------------------------------- 7. head exhaustion
SMALL_K = (0, 1, 3, 4, 5)


def head_exhaustion():
    """Lists around the length of the staged head (K - 1, K, K + 1, K + 5) whose first m entries of the sorted order belong to earlier queries
    (m = 0, K - 1, K, K + 1, all but one), with and without gated entries (which sort last: the staged head then ends in a sentinel)."""
    cases = []
    ratio = 0.8
    for K in SMALL_K:
        B = Builder(70 + K)
        for n in sorted({max(1, K - 1), max(1, K), K + 1, K + 5}):
            for m in sorted({x for x in (0, K - 1, K, K + 1, n - 1) if 0 <= x < n}):
                for n_gated in (0, 2):
                    ds = [20 + 7 * j for j in range(n)]  # sorted order; listed in reverse scan order
                    ts = [B.target() for _ in range(n)]
                    for j in range(m):
                        B.query([(ts[j], 5)], expect=ts[j])  # an earlier query owns sorted entry j
                    second = ds[m + 1] if m + 1 < n else MAX_HAMMING_DIST
                    ent = [(B.target(), 8, 1) for _ in range(n_gated)] + [(ts[j], ds[j]) for j in reversed(range(n))]
                    B.query(ent, expect=ts[m] if accepts(ds[m], second, ratio) else -1)
        cases.append(B.build(f"head_exhaustion/K{K}", RATIO, 100, ratio, K=K))
    return cases


# ---------------------------------------------------------------------------------------------------- 8. claim chains
def _chain(B, n, invalid=()):
    """query 0 lists target 1; query i lists target i (10 bits) and target i + 1 (30 bits): every query's best is taken by its predecessor"""
    ts = [B.target() for _ in range(n + 1)]
    shifted = True  # does query i still lose its best to query i - 1?
    for i in range(n):
        valid = i not in invalid
        ent = [(ts[1], 10)] if i == 0 else [(ts[i], 10), (ts[i + 1], 30)]
        exp = -1 if not valid else ts[i + 1] if shifted else ts[i]
        if not valid:
            shifted = False  # an invalid query claims nothing: its successor keeps its own best, and so does everyone after
        B.query(ent, expect=exp, valid=int(valid))
    return ts


def claim_chains():
    cases = []
    for mode in (BEST_ONLY, RATIO):
        B = Builder(80 + mode)
        _chain(B, 40)
        cases.append(B.build(f"claim_chains/inside_chunk/{MODE_NAMES[mode]}", mode, 100, 0.8, q_start=0, chain=40))
        B = Builder(82 + mode)
        _chain(B, 40)
        cases.append(B.build(f"claim_chains/across_1024/{MODE_NAMES[mode]}", mode, 100, 0.8, q_start=1004, chain=40))
    B = Builder(85)
    _chain(B, 40, invalid=(10, 25))
    cases.append(B.build("claim_chains/invalid_inside", RATIO, 100, 0.8, q_start=1004, chain=10))
    # queries of the second chunk whose best and second were closed by the first chunk (shared targets: distance = a[q] + b[t])
    B = Builder(86, additive=([3, 1, 8, 10, 20], [2, 4, 6, 30]))
    t1, t2, t3, t4 = (B.target() for _ in range(4))
    B.query([(t1, 5)], expect=t1)
    B.query([(t2, 5)], expect=t2)
    B.query([(t1, 10), (t2, 12), (t3, 14)], expect=t3)
    B.query([(t2, 14), (t1, 12), (t3, 16), (t4, 40)], expect=t4)
    B.query([(t1, 22), (t2, 24), (t3, 26), (t4, 50)], expect=-1)
    cases.append(B.build("claim_chains/closed_by_chunk_1", RATIO, 100, 0.8, q_at=[1000, 1001, 1030, 1031, 1100], chain=1))
    return cases


# ---------------------------------------------------------------------------------------------------- 9. area
def area():
    cases = []
    thr, ratio = 50, 0.9
    B = Builder(91)
    t = B.target()
    B.query([(t, 30)], expect=-1)      # holds t until query 2 comes
    B.query([(t, 30)], expect=-1)      # equally close: the holder keeps it
    B.query([(t, 29)], expect=t)       # strictly closer: takes it, query 0 is cleared
    B.query([(t, 29)], expect=-1)
    ta, tb = B.target(), B.target()
    B.query([(ta, 20)], expect=-1)            # holds ta until query 6 takes it
    B.query([(ta, 25), (tb, 30)], expect=tb)  # ta is held closer: not even a second
    B.query([(B.target(), 28), (ta, 19)], expect=ta)  # 19 < 20: a candidate again; 0.9 * 28 = 25.2 >= 19: takes ta from query 4
    cases.append(B.build("area/take_over", AREA, thr, ratio))
    B = Builder(92)
    t = B.target()
    for i in range(10):
        B.query([(t, 40 - i)], expect=t if i == 9 else -1)  # every query takes the target from its predecessor
    t = B.target()
    for i in range(10):
        B.query([(t, 31 + i)], expect=t if i == 0 else -1)  # ... and nobody does when the distances grow
    cases.append(B.build("area/chain_of_10", AREA, thr, ratio, q_start=1019))
    B = Builder(93)  # best and second on the same lane's share (64 apart) and on different lanes
    for pb, ps in ((0, 64), (64, 0), (0, 65), (65, 0), (3, 70), (63, 64), (1, 129)):
        for second in (44, 45):  # 0.9 * 44 = 39.6 < 40: rejected; 40.5: accepted
            L = max(pb, ps) + 2
            ent, tbest = [], None
            for p in range(L):
                if p == pb:
                    tbest = B.target()
                    ent.append((tbest, 40))
                elif p == ps:
                    ent.append((B.target(), second))
                else:
                    ent += B.fars(1)
            B.query(ent, expect=tbest if second == 45 else -1)
    cases.append(B.build("area/second_on_another_lane", AREA, thr, ratio))
    return cases


CLASSES = {"threshold": threshold, "ratio_equality": ratio_equality, "same_octave": same_octave, "triangulation_order": triangulation_order,
           "ties": ties, "gates": gates, "head_exhaustion": head_exhaustion, "claim_chains": claim_chains, "area": area}
# the deliberate mistakes every class has to catch (head_stop takes the K of the case)
SENSITIVITY = {"threshold": ("thr_le", "tri_start_256"), "ratio_equality": ("ratio_le",), "same_octave": ("ignore_levels", "prune_thr_only"),
               "triangulation_order": ("tri_sorted",), "ties": ("later_tie",), "gates": ("gate30_ge", "xright_ge0", "tol_le"),
               "head_exhaustion": ("head_stop",), "claim_chains": ("chunk_blind",), "area": ("area_le",)}


@functools.lru_cache(maxsize=None)
def cases_of(cls):
    return tuple(CLASSES[cls]())
