"""The planted stereo problems of tests/stereo_problems.py, on the CPU: the numpy restatement, the C oracle and -- where
oracle/_ref/libsvref.so was built -- the reference's own match/stereo.cc agree bit for bit on every class, and every class reaches the
boundary sides its docstring names (asserted on the restatement's reason codes and intermediates, not on outputs alone)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import stereo_problems as SP

_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libsvref.so")
CLASSES = list(SP.all_classes())


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(_SO):
        pytest.skip("oracle/_ref/libsvref.so absent: it is built from /root/reference by `make -C oracle/ref_local` (build container only)")
    return C.CDLL(_SO)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _reference(ref, p):
    pl, pr = p.pyramids()
    L = len(pl)
    PL = (C.c_void_p * L)(*[a.ctypes.data for a in pl])
    PR = (C.c_void_p * L)(*[a.ctypes.data for a in pr])
    lw = np.array([a.shape[1] for a in pl], np.int32)
    lh = np.array([a.shape[0] for a in pl], np.int32)
    lsl = np.array([a.strides[0] for a in pl], np.int32)
    lsr = np.array([a.strides[0] for a in pr], np.int32)
    kl, kr = np.ascontiguousarray(p.kl), np.ascontiguousarray(p.kr)
    dl, dr = np.ascontiguousarray(p.dl, np.uint8), np.ascontiguousarray(p.dr, np.uint8)
    xr, dp = np.zeros(max(len(kl), 1), np.float32), np.zeros(max(len(kl), 1), np.float32)
    ref.svref_stereo_compute.restype = None
    ref.svref_stereo_compute(_p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr), PL, PR, _p(lw), _p(lh), _p(lsl), _p(lsr), C.c_float(p.scale_factor), L,
                             C.c_float(p.fxb), C.c_float(p.baseline), _p(xr), _p(dp))
    return xr[:len(kl)], dp[:len(kl)]


@pytest.mark.parametrize("name", CLASSES)
def test_restatement_equals_oracle(name):
    for p in SP.problems(name):
        r = p.restate()
        xo, do = p.oracle()
        assert np.array_equal(_bits(r["stereo_x_right"]), _bits(xo)) and np.array_equal(_bits(r["depth"]), _bits(do)), p.name
        # the two outputs move together, and -1 is never a result
        assert np.array_equal(xo == -1, do == -1) and np.array_equal(xo == -1, ~np.isin(r["reason"], (SP.KEPT, SP.CLAMPED))), p.name


@pytest.mark.parametrize("name", CLASSES)
def test_oracle_equals_reference(ref, name):
    for p in SP.problems(name):
        if len(p.kl) == 0:
            continue  # nothing to compare: the reference returns two empty vectors
        xo, do = p.oracle()
        xr, dp = _reference(ref, p)
        assert np.array_equal(_bits(xr), _bits(xo)) and np.array_equal(_bits(dp), _bits(do)), p.name


@pytest.mark.parametrize("name", CLASSES)
def test_class_reaches_what_it_names(name):
    for p in SP.problems(name):
        r = p.restate()
        planted_kept = finally_kept = 0
        for tag, (il, want) in p.info["expect"].items():
            if tag.endswith("_winner"):
                assert r["best_idx"][il] == want, (p.name, tag, r["best_idx"][il])
            elif tag.endswith("_min_candidates"):
                assert r["n_row"][il] > want, (p.name, tag, r["n_row"][il])
            else:
                got = r["pre_reason"][il] if p.info.get("textured") and want == SP.KEPT else r["reason"][il]
                assert got == want, (p.name, tag, SP.REASONS[got], SP.REASONS[want])
                planted_kept += want in (SP.KEPT, SP.CLAMPED)
                finally_kept += want in (SP.KEPT, SP.CLAMPED) and r["reason"][il] in (SP.KEPT, SP.CLAMPED)
        assert 5 * finally_kept >= 4 * planted_kept, (p.name, finally_kept, planted_kept)
        n_kept = int(np.isin(r["reason"], (SP.KEPT, SP.CLAMPED)).sum())
        assert (n_kept == 0) if p.rejecting else (n_kept > 0), (p.name, n_kept)


# ---------------------------------------------------------------------------------------------------- per class: the intermediates
def _r(name, i=0):
    p = SP.problems(name)[i]
    return p, p.restate(), p.info["expect"]


def test_hamming_gate_distances_and_ties():
    p, r, e = _r("hamming_gate")
    assert r["best_dist"][e["d74"][0]] == 74 and r["best_dist"][e["d75"][0]] == 75 and r["best_idx"][e["d75"][0]] == -1
    for tag, copies in (("tie2", 2), ("tie3", 3)):
        il, win = e[tag][0], e[tag + "_winner"][1]
        same = [i for i in range(len(p.kr)) if np.array_equal(p.dr[i], p.dr[win])]
        assert len(same) == copies and min(same) == win and win > 0
        d = np.unpackbits(p.dr ^ p.dl[il], axis=1).sum(1)
        closer = np.nonzero(d < d[win])[0]
        assert len(closer) == 1 and abs(int(p.kr["octave"][closer[0]]) - int(p.kl["octave"][il])) == 2   # closer, but gated by its octave
        assert any(d[i] > d[win] and d[i] < SP.HAMMING_THR for i in range(win))                              # a worse candidate stored before it


def test_level_gate_octaves():
    p, r, e = _r("level_gate")
    L = p.num_levels
    seen = {(int(p.kl["octave"][il]), int(p.kr["octave"][il])) for il, _ in e.values()}   # probe i owns right keypoint i
    assert seen == {(0, 0), (0, 1), (0, 2), (L - 1, L - 3), (L - 1, L - 2), (L - 1, L - 1)}


def test_disparity_gate_ulps():
    p, r, e = _r("disparity_gate")
    xl, md = np.float32(150), r["max_disp"]
    assert md == 64 and np.float32(np.float32(p.fxb) / np.float32(p.baseline)) == md
    x = {t: p.kr["x"][e[t][0]] for t in ("at_min", "below_min", "at_max", "above_max")}
    assert x["at_min"] == xl - md and x["below_min"] == np.nextafter(xl - md, np.float32(0))
    assert x["at_max"] == xl and x["above_max"] == np.nextafter(xl, np.float32(1e9))
    assert r["best_idx"][e["below_min"][0]] == -1 and r["best_idx"][e["above_max"][0]] == -1


def test_row_bands_edges():
    p, r, e = _r("row_bands")
    sf = O.scale_tables(p.scale_factor, p.num_levels)[0]
    rad = np.float32(2.0) * sf[p.kr["octave"]]
    lo = np.floor((p.kr["y"] - rad).astype(np.float64)).astype(int)
    hi = np.ceil((p.kr["y"] + rad).astype(np.float64)).astype(int)
    assert lo.min() == 0 and hi.max() == p.left.shape[0] - 1
    assert ((p.kr["y"] - rad) == lo).any() and ((p.kr["y"] + rad) == hi).any()          # exactly integral band ends
    for tag in ("int", "above", "below"):
        for side, n in (("lo_out", 0), ("lo_in", 1), ("hi_in", 1), ("hi_out", 0)):
            il = e[f"{tag}_{side}"][0]
            assert p.kl["y"][il] != np.floor(p.kl["y"][il])                              # fractional: the row is the truncation
            assert (r["n_row"][il] > 0) == bool(n), (tag, side)
    assert r["n_row"][e["row65"][0]] > 64 and r["n_row"][e["row257"][0]] > 256


def test_rounding_halves_are_halves():
    p, r, e = _r("rounding_halves")
    frac = lambda v: float(v) - np.floor(float(v))
    par = lambda v: int(np.floor(float(v))) % 2
    seen = set()
    for tag, (il, _) in e.items():
        ir = r["best_idx"][il]
        for what, v in (("xl", p.kl["x"][il]), ("yl", p.kl["y"][il]), ("xr", p.kr["x"][ir])):
            if frac(v) == 0.5:
                seen.add((what, par(v)))
    assert seen == {(w, k) for w in ("xl", "yl", "xr") for k in (0, 1)}


def test_window_borders_positions():
    p, r, e = _r("window_borders")
    isf = O.scale_tables(p.scale_factor, p.num_levels)[1]
    sizes = O.level_sizes(p.left.shape[1], p.left.shape[0], p.scale_factor, p.num_levels)
    rnd = lambda v, l: int(np.rint(np.float32(np.float32(v) * isf[l])))
    for l, (w, h) in enumerate(sizes):
        for tag, want in (("ini0", 10), ("ini-1", 9), ("end_w-1", w - 11), ("end_w", w - 10)):
            il = e[f"L{l}_{tag}"][0]
            assert p.kl["octave"][il] == l and rnd(p.kr["x"][il], l) == want, (l, tag)
        assert rnd(p.kl["y"][e[f"L{l}_syl-5"][0]], l) == 5 and rnd(p.kl["y"][e[f"L{l}_syl+5"][0]], l) == h - 6
    assert rnd(p.kl["x"][e["L0_sxl+5"][0]], 0) == sizes[0][0] - 6 and rnd(p.kl["x"][e["L0_sxl-5"][0]], 0) == 5


def test_correlation_shapes_profiles():
    p, r, e = _r("correlation_shapes")
    off = {t: int(r["best_off"][e[t][0]]) for t in e}
    assert (off["off-5"], off["off+5"], off["off-4"], off["off+4"], off["tie"]) == (-5, 5, -4, 4, -2)
    c = r["corr"][e["tie"][0]]
    assert list(c) == p.info["tie"] and c[3] == c[5] == c.min()
    c = r["corr"][e["c3==c2"][0]]
    assert c[5] == c[6] == c.min() and r["x_delta"][e["c3==c2"][0]] == 0.5
    assert (r["corr"][e["constant"][0]] == 0).all()
    c = r["corr"][e["saturated"][0]]
    assert list(c) == p.info["saturated"] and c.min() > 32767 and r["pre_reason"][e["saturated"][0]] == SP.KEPT


def test_disparity_results_values():
    for i, name in enumerate(("equal", "ulp_below")):
        p, r, e = _r("disparity_results", i)
        d = r["disp"][e["at_max_disp"][0]]
        assert (d == r["max_disp"]) if name == "equal" else (d == np.nextafter(r["max_disp"], np.float32(0)))
        z = e["zero"][0]
        assert r["disp"][z] == 0 and r["stereo_x_right"][z] == np.float32(p.kl["x"][z] - np.float32(0.01))
        assert r["disp"][e["negative"][0]] < 0


def test_median_sets_values():
    sizes = {}
    for p in SP.problems("median_sets"):
        r = p.restate()
        sizes[p.name[12:]] = r["n_kept_before_median"]
        assert r["median"] == p.info["median"] and (r["reason"] == SP.MEDIAN_DROPPED).sum() == p.info["dropped"], p.name
    assert [sizes[k] for k in ("size0", "size1", "size2", "size3", "size8")] == [0, 1, 2, 3, 8]
    assert sizes["median0"] == 5 and sizes["twice"] == 5


def test_many_left_sizes_and_median():
    base, a, b = SP.problems("many_left")
    assert (len(a.kl), len(b.kl)) == (32768, 32769)
    ma, mb, m0 = a.restate()["median"], b.restate()["median"], base.restate()["median"]
    assert ma == a.info["high_min"] and mb == b.info["low_max"] and ma != m0 and mb != m0   # the last keypoint alone moves the median
    assert (b.restate()["reason"][:32768] == SP.MEDIAN_DROPPED).sum() > (a.restate()["reason"] == SP.MEDIAN_DROPPED).sum() > 0


def test_index_limit_last_index():
    p, r, e = _r("index_limit")
    assert len(p.kr) == 65535 and r["best_idx"][0] == 65534 and r["n_row"][0] > 1000
    d = np.unpackbits(p.dr ^ p.dl[0], axis=1).sum(1)
    closer = np.nonzero(d < d[65534])[0]
    assert set(closer) >= {65534 & 0x7FFF, 65534 & 0x3FFF}      # what a narrower index mask would pick instead


def test_tall_rows_and_other_pyramid_bands():
    for p in SP.problems("tall"):
        h = p.left.shape[0]
        rows = p.kl["y"].astype(int)
        assert rows.max() == h - 6 and (h <= 1030 or {1022, 1023, 1024, 1025} <= set(rows)) and (h <= 2040 or rows.max() > 2040)
        assert np.ceil(p.kr["y"] + 2).max() == h - 1
    for p in SP.problems("other_pyramids"):
        assert p.info["widest"] == p.info["rows_per_kp"] - 1    # the widest band the level can have; the list has one row to spare
        assert set(p.kl["octave"]) == set(range(p.num_levels))
