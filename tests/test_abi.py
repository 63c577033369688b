"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/svgpu.h declares, carries the signatures the header
declares, reports errors instead of crashing without a device, and its host-only arithmetic agrees with the oracle.
No compute kernels are launched here."""
import ctypes as C
import mmap
import pathlib
import re

import numpy as np
import pytest

from oracle import oracle as O

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def L():
    from stella_vslam_amd import _lib
    _lib.build()
    return _lib.lib()


def test_every_declared_symbol_is_exported(L):
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    names = sorted(set(re.findall(r"^(?:int|void|void\*|const char\*)\s+(svgpu_[a-z0-9_]+)\s*\(", hdr, flags=re.M)))
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), n
    assert L.svgpu_abi_version() == 1


def test_header_cites_reference_interfaces():
    hdr = (ROOT / "include" / "svgpu.h").read_text()
    for cite in ("feature/orb_extractor.h:46-71", "match/robust.cc:232-328", "match/projection.cc:13-93",
                 "optimize/local_bundle_adjuster.h:23", "match/base.h:20-41"):
        assert cite in hdr


def test_errors_not_crashes_without_device(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert L.svgpu_create(0, C.byref(h)) == 5  # SVGPU_ERR_NO_DEVICE
    assert L.svgpu_device_count() == 0
    assert L.svgpu_status_string(5).decode() == "no HIP device"
    assert L.svgpu_orb_max_keypoints(None) == -1
    assert L.svgpu_orb_extract(None, None, 0, None, 0, None, None, 0, None, None) == 1  # SVGPU_ERR_INVALID
    assert L.svgpu_local_ba(None, None, None, None, None, None, None) == 1


def test_product_has_no_cpu_fallback_and_no_oracle_dependency():
    """Nothing under stella_vslam_amd/ may import, link or load the oracle."""
    pkg = ROOT / "stella_vslam_amd"
    pat = re.compile(r"from\s+oracle|import\s+oracle|liboracle|oracle/[a-z_]+\.(c|py|so)|orc_[a-z_]+\(")
    for f in list(pkg.rglob("*.py")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.h")) + list(pkg.rglob("*.cpp")) + list(pkg.rglob("Makefile")):
        m = pat.search(f.read_text())
        assert m is None, (f, m.group(0))


def test_scale_tables_host_function_matches_oracle_and_reference_test(L):
    for sf, n in ((1.2, 8), (1.26, 10), (2.0, 4)):
        tabs = [np.zeros(n, np.float32) for _ in range(4)]
        assert L.svgpu_orb_scale_tables(C.c_float(sf), n, *[t.ctypes.data_as(C.c_void_p) for t in tabs]) == 0
        for a, b in zip(tabs, O.scale_tables(sf, n)):
            assert np.array_equal(a, b)
    assert L.svgpu_orb_scale_tables(C.c_float(1.2), 0, None, None, None, None) == 1


# ------------------------------------------------------------------------------------------- signatures derived from the header
RESTYPES = {"int": C.c_int, "void": None, "void*": C.c_void_p, "const char*": C.c_char_p}


def _declared():
    """{name: (return type as written, parameter count)} by the header regex above and a count of the top-level commas -- written
    without the parser under test."""
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", " ", (ROOT / "include" / "svgpu.h").read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"^(int|void|void\*|const char\*)\s+(svgpu_[a-z0-9_]+)\s*\(", hdr, flags=re.M):
        depth, commas, i = 1, 0, m.end()
        while depth:
            depth += (hdr[i] == "(") - (hdr[i] == ")")
            commas += hdr[i] == "," and depth == 1
            i += 1
        inner = hdr[m.end():i - 1].strip()
        out[m.group(2)] = (m.group(1), 0 if inner in ("", "void") else commas + 1)
    return out


def test_every_declared_function_carries_its_signature(L):
    decl = _declared()
    assert len(decl) >= 125
    for name, (ret, nparams) in decl.items():
        fn = getattr(L, name)
        assert isinstance(fn.argtypes, list) and len(fn.argtypes) == nparams, name
        assert fn.restype is RESTYPES[ret], name


def test_derived_signatures_equal_the_ones_written_by_hand(L):
    """The 17 signatures the binding declared by hand before it read the header, as they stood."""
    vp, i32 = C.c_void_p, C.c_int
    hand = {
        "svgpu_pose_graph_optimize": (C.c_int, [vp, i32, vp, vp, i32, vp, vp, vp, i32, i32, C.c_double, vp, vp, vp]),
        "svgpu_pose_graph_optimize_ex": (C.c_int, [vp, i32, vp, vp, i32, vp, vp, vp, i32, i32, C.c_double, vp, vp, vp, vp, vp]),
        "svgpu_selftest_pose_graph_envelope_solve": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "svgpu_pose_graph_correct_landmarks": (C.c_int, [vp, i32, vp, vp, i32, vp, vp, vp]),
        "svgpu_sim3_transform_optimize_batch": (C.c_int, [vp, i32, vp, i32] + [vp] * 9 + [C.c_float, i32, i32, vp, vp, vp, vp]),
        "svgpu_sim3_transform_optimize": (C.c_int, [vp, vp, vp, i32] + [vp] * 7 + [C.c_float, i32, i32, vp, vp, vp, vp]),
        "svgpu_pose_optimize_batch": (C.c_int, [vp, i32] + [vp] * 9 + [i32] * 4 + [vp] * 4),
        "svgpu_selftest_cand_replay_form": (C.c_int, [i32, i32, i32, i32]),
        "svgpu_ingest_gray_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
        "svgpu_ingest_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "svgpu_ingest_destroy": (None, [C.c_void_p]),
        "svgpu_ingest_gray": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
        "svgpu_ingest_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int]),
        "svgpu_ingest_depth_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p]),
        "svgpu_tracker_set_ingest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double]),
    }
    for name, (restype, argtypes) in hand.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    # the three the hand-written block gave a return type only
    assert L.svgpu_last_error.restype is C.c_char_p and L.svgpu_status_string.restype is C.c_char_p and L.svgpu_stream.restype is C.c_void_p


def test_parse_header_is_a_pure_function_of_the_text():
    from stella_vslam_amd._lib import parse_header
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    text = """
        typedef struct svgpu_ctx svgpu_ctx;
        typedef int (*svgpu_allreduce_fn)(void* user, double* dev_buf, size_t count, void* stream);
        int svgpu_multi_line(svgpu_ctx* ctx, const float* a,
                             int n,
                             double w, size_t bytes);
        int svgpu_block_comments(int a /* first */, /* second, with a comma */ float b, unsigned c /* last */);
        int svgpu_line_comments(int a,   // first, with a comma
                                int32_t b  // second
                                );
        int svgpu_pointer_to_pointer(svgpu_ctx** out, const double** rows);
        int svgpu_volatile_flag(volatile uint8_t* stop);
        int svgpu_inline_callback(int n, int (*reduce)(void* user, double* buf, size_t count, void* stream), void* user);
        int svgpu_named_callback(svgpu_allreduce_fn reduce, void* user);
        void svgpu_returns_nothing(svgpu_ctx* ctx);
        int svgpu_takes_nothing(void);
        void* svgpu_returns_pointer(svgpu_ctx* ctx);
        const char* svgpu_returns_text(const svgpu_ctx* ctx, const char* key);
    """
    assert parse_header(text) == {
        "svgpu_multi_line": (C.c_int, [vp, vp, i32, C.c_double, C.c_size_t]),
        "svgpu_block_comments": (C.c_int, [i32, f32, C.c_uint]),
        "svgpu_line_comments": (C.c_int, [i32, C.c_int32]),
        "svgpu_pointer_to_pointer": (C.c_int, [vp, vp]),
        "svgpu_volatile_flag": (C.c_int, [vp]),
        "svgpu_inline_callback": (C.c_int, [i32, vp, vp]),
        "svgpu_named_callback": (C.c_int, [vp, vp]),
        "svgpu_returns_nothing": (None, [vp]),
        "svgpu_takes_nothing": (C.c_int, []),
        "svgpu_returns_pointer": (vp, [vp]),
        "svgpu_returns_text": (C.c_char_p, [vp, C.c_char_p]),
    }
    with pytest.raises(ValueError, match=r"svgpu_wide.*long double"):
        parse_header("int svgpu_wide(svgpu_ctx* ctx, long double x);")
    with pytest.raises(ValueError, match=r"svgpu_wide_return.*long long"):
        parse_header("long long svgpu_wide_return(void);")


def _above_4g(a):
    """a copy of `a` whose address does not fit 32 bits: numpy's own allocation where it already lies there, else anonymous mappings
    until one does (kept alive by the array that views them)"""
    a = np.array(a)
    held = []
    while a.ctypes.data < 2 ** 32:
        held.append(mmap.mmap(-1, max(a.nbytes, mmap.PAGESIZE)))
        b = np.frombuffer(held[-1], a.dtype, a.size).reshape(a.shape)
        b[...] = a
        a = b
    assert a.ctypes.data >= 2 ** 32
    return a


def test_pointers_arrive_whole_without_wrappers(L):
    """Plain Python floats and ints and raw 64-bit addresses, no ctypes wrapper anywhere: the derived signatures carry them."""
    for sf, n in ((1.2, 8), (1.26, 10), (2.0, 4)):
        tabs = [_above_4g(np.zeros(n, np.float32)) for _ in range(4)]
        assert L.svgpu_orb_scale_tables(sf, n, *[t.ctypes.data for t in tabs]) == 0
        for a, b in zip(tabs, O.scale_tables(sf, n)):
            assert np.array_equal(a, b)
    ocam = O.make_camera(O.CAM_PERSPECTIVE, 640, 480, 400.0, 410.0, 320.0, 240.0, (-0.1, 0.01, 0.0, 0.0, 0.0))
    cam = _above_4g(np.frombuffer(bytes(ocam), np.uint8))  # svgpu_camera has the oracle Camera's layout
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    for trans, pos in (([0.1, -0.2, 0.3], [0.5, 0.4, 3.0]), ([0.0, 0.0, 0.0], [-1.0, 2.0, 7.5]), ([0.1, -0.2, 0.3], [0.2, 0.1, -4.0])):
        R, t, p, b = (_above_4g(np.asarray(x, np.float64)) for x in (rot, trans, pos, np.zeros(3)))
        valid = _above_4g(np.full(1, -1, np.int32))
        assert L.svgpu_reproject_to_bearing(cam.ctypes.data, R.ctypes.data, t.ctypes.data, p.ctypes.data, b.ctypes.data, valid.ctypes.data) == 0
        eb, ev = O.reproject_to_bearing(ocam, rot, trans, pos)
        assert np.array_equal(b, eb) and bool(valid[0]) == ev


def test_a_missing_argument_never_enters_the_library(L):
    """(ctypes lets surplus arguments of a cdecl function through, as C does for a variadic one: only a missing one is caught)"""
    tabs = [np.full(4, 7, np.float32) for _ in range(4)]
    with pytest.raises(TypeError):
        L.svgpu_orb_scale_tables(1.2, 4, *[t.ctypes.data for t in tabs[:3]])
    assert all((t == 7).all() for t in tabs)
