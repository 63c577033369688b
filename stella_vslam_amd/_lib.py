"""Loader of the C-ABI shared library (stella_vslam_amd/libsvgpu.so).

There is NO fallback: if the HIP library is missing or fails to load, importing the product path
raises.  (The CPU oracle under oracle/ is test infrastructure and is never used here.)

The signature of every function is read from include/svgpu.h when the library is loaded (parse_header): ctypes then converts
plain Python ints and floats to the declared C types, passes every pointer at full width and refuses a call that leaves
an argument out.
"""
from __future__ import annotations

import ctypes as C
import pathlib
import re
import subprocess

import os

_HERE = pathlib.Path(__file__).resolve().parent
# SVGPU_LIB_PATH selects an A/B build of the SAME library (tools/build_variant.sh) for kernel experiments; there is still no fallback
LIB_PATH = pathlib.Path(os.environ["SVGPU_LIB_PATH"]) if os.environ.get("SVGPU_LIB_PATH") else _HERE / "libsvgpu.so"
HEADER_PATH = _HERE.parent / "include" / "svgpu.h"
_LIB = None


class SvgpuError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: svgpu status {status} ({status_string(status)}) {detail}".rstrip())


def build(force: bool = False) -> pathlib.Path:
    """(Re)build libsvgpu.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    srcs = list((_HERE / "csrc").glob("*.hip")) + list((_HERE / "csrc").glob("*.h")) + list((_HERE / "csrc").glob("*.inc"))
    srcs.append(HEADER_PATH)
    stale = force or not LIB_PATH.exists() or any(s.stat().st_mtime > LIB_PATH.stat().st_mtime for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", str(_HERE / "csrc"), "-j8"] + (["-B"] if force else []))
    return LIB_PATH


# Every pointer (T*, T**, opaque handles, function pointers) is a c_void_p: its from_param takes None, an int, bytes, a c_void_p,
# byref(...), data_as(...) results, ctypes arrays and CFUNCTYPE objects.  Only `const char*` is a c_char_p.
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "svgpu_allreduce_fn": C.c_void_p}
_DECL = re.compile(r"([\w\s*]+?)\b(svgpu_\w+)\s*\(((?:[^()]|\([^()]*\))*)\)\s*;")


def _ctype(decl: str, name: str, is_param: bool):
    """ctypes type of one parameter (`const float* x`) or return type (`void*`) of function `name`"""
    t = re.sub(r"\s*\*\s*", "* ", " ".join(decl.split())).strip()
    if "*" in t:  # every pointer, an inline function pointer included
        return C.c_char_p if re.fullmatch(r"const char\*( \w+)?", t) else C.c_void_p
    words = [w for w in t.split() if w != "const"]
    t = " ".join(words[:-1] if is_param and len(words) > 1 else words)  # (without the parameter's name)
    if t in _SCALARS or (t == "void" and not is_param):
        return _SCALARS.get(t)
    raise ValueError(f"{name}: no ctypes mapping for the {'parameter' if is_param else 'return'} type `{t}`")


def parse_header(text: str) -> dict:
    """{name: (restype, [argtypes])} of every svgpu_* function the header text declares.  A type outside the fixed mapping is a
    ValueError naming the function and the type."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.S | re.M)
    out = {}
    for ret, name, params in _DECL.findall(text):
        params = [] if params.strip() in ("", "void") else re.split(r",(?![^()]*\))", params)  # at the top-level commas
        out[name] = (_ctype(ret, name, False), [_ctype(p, name, True) for p in params])
    return out


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not LIB_PATH.exists():
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        if not HEADER_PATH.exists():
            raise ImportError(f"{HEADER_PATH} is missing: the binding reads its C signatures from it")
        L = C.CDLL(str(LIB_PATH))
        try:
            for name, (restype, argtypes) in parse_header(HEADER_PATH.read_text()).items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        except (ValueError, AttributeError) as e:
            raise ImportError(f"{HEADER_PATH} does not match {LIB_PATH}: {e}") from e
        if L.svgpu_abi_version() != 1:
            raise ImportError("libsvgpu.so ABI version mismatch")
        _LIB = L
    return _LIB


def ptr(a):
    """What a pointer parameter takes for `a`: None, a host numpy array, a device tensor (anything with data_ptr()) or an address.
    The numpy form keeps its array alive, so a temporary may be converted inside the call expression."""
    if a is None:
        return None
    view = getattr(a, "ctypes", None)  # (numpy builds this object on every access: once)
    if view is not None:
        return view.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else int(a))


def status_string(status: int) -> str:
    try:
        return lib().svgpu_status_string(status).decode()
    except Exception:
        return "?"
