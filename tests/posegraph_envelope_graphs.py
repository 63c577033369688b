"""Graphs of the envelope planner's tests (stella_vslam_amd/csrc/posegraph_envelope_plan.h), shared by the CPU check
(tests/test_posegraph_envelope.py) and the device self-test (tests/test_gpu_posegraph_direct.py), and the driver of
tests/posegraph_envelope_check.cpp.  A graph is (nfree, edges): edges is a list of (a, b) free slots, -1 for a fixed end."""
from __future__ import annotations

import functools
import pathlib
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent


def chain(n, window=3, loop=True):
    """Slots 0 .. n - 1, every slot joined to its `window` predecessors, and one far loop pair (n - 1, 0) where that is not a chain pair."""
    edges = [(k, k - d) for k in range(1, n) for d in range(1, window + 1) if k - d >= 0]
    if loop and n - 1 > window:
        edges.append((n - 1, 0))
    return n, edges


def ring(n):
    return n, [((k + d) % n, k) for k in range(n) for d in (1, 2)]


def hub(leaves=40):
    return leaves + 1, [(k, 0) for k in range(1, leaves + 1)]


def dense(n=70):
    """Every pair: each column is as tall as it can be (69 rows in the first one, more than a wavefront)."""
    return n, [(a, b) for a in range(n) for b in range(a)]


def duplicates():
    n, edges = 6, [((k + 1) % 6, k) for k in range(6)]
    return n, edges[:2] + [(2, 1), (1, 2), (2, 1)] + edges[2:]


def two_components():
    n1, e1 = ring(9)
    n2, e2 = chain(7, 2)
    return n1 + n2, e1 + [(a + n1, b + n1) for a, b in e2]


def from_problem(p):
    """The free-slot graph of a pose-graph problem (tests/posegraph_problems.py): fixed vertices vanish, their edges keep a -1 end."""
    fixed = p["fixed"].astype(bool)
    slot = np.where(fixed, -1, np.cumsum(~fixed) - 1)
    return int((~fixed).sum()), [(int(slot[a]), int(slot[b])) for a, b in zip(p["e1"], p["e2"])]


def envelope_blocks(nfree, edges, order):
    """Blocks of the lower envelope (diagonal included) when slot order[p] sits at position p."""
    pos = np.empty(nfree, int)
    pos[np.asarray(order, int)] = np.arange(nfree)
    first = np.arange(nfree)
    for a, b in edges:
        if a >= 0 and b >= 0 and a != b:
            lo, hi = sorted((pos[a], pos[b]))
            first[hi] = min(first[hi], lo)
    return int((np.arange(nfree) - first + 1).sum())


def natural_and_interleaved(nfree, edges):
    inter = np.empty(nfree, int)
    inter[0::2] = np.arange((nfree + 1) // 2)
    inter[1::2] = nfree - 1 - np.arange(nfree // 2)
    return envelope_blocks(nfree, edges, np.arange(nfree)), envelope_blocks(nfree, edges, inter)


@functools.lru_cache(maxsize=None)
def check_program():
    cxx = shutil.which("g++")
    if cxx is None:
        raise RuntimeError("g++ is needed to build tests/posegraph_envelope_check.cpp")
    exe = pathlib.Path(tempfile.mkdtemp(prefix="pg_env_check_")) / "posegraph_envelope_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "stella_vslam_amd" / "csrc"),
                           str(ROOT / "tests" / "posegraph_envelope_check.cpp"), "-o", str(exe)])
    return exe


def run_check(nfree, edges):
    """Runs the check program on the graph.  Returns (returncode, stdout, dict blocks / max_column_rows / ordering / residual)."""
    nat, inter = natural_and_interleaved(nfree, edges)
    exe = check_program()
    path = exe.parent / f"graph_{nfree}_{len(edges)}_{abs(hash(tuple(edges))) % 10 ** 9}.txt"
    path.write_text(f"{nfree} {len(edges)} {nat} {inter}\n" + "".join(f"{a} {b}\n" for a, b in edges))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    info = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w and w[0] == "PLAN":
            info.update(blocks=int(w[1]), max_column_rows=int(w[2]), ordering=int(w[3]))
        if w and w[0] == "RESIDUAL":
            info["residual"] = float(w[1])
    info.update(natural=nat, interleaved=inter)
    return r.returncode, r.stdout + r.stderr, info


# ---- the self-test's system on a graph: the deterministic, strictly diagonally dominant blocks of the check program
def system(nfree, edges):
    """(pair_a, pair_b, diag_blocks, pair_blocks, rhs) over the DISTINCT unordered pairs of the graph (lo, hi ascending)."""
    pairs = sorted({(min(a, b), max(a, b)) for a, b in edges if a >= 0 and b >= 0 and a != b})
    k = np.arange(len(pairs))[:, None, None]
    r, c = np.arange(7)[None, :, None], np.arange(7)[None, None, :]
    blocks = (((k * 49 + r * 7 + c) * 37 + 11) % 101) / 101.0 - 0.5
    s = np.arange(nfree)[:, None, None]
    diag = (((s * 49 + np.minimum(r, c) * 7 + np.maximum(r, c)) * 53 + 29) % 103) / 103.0 - 0.5
    rowsum = np.abs(diag).sum(2) - np.abs(diag[:, np.arange(7), np.arange(7)])
    pa = np.array([p[0] for p in pairs], np.int32)
    pb = np.array([p[1] for p in pairs], np.int32)
    if len(pairs):
        np.add.at(rowsum, pa, np.abs(blocks).sum(2))
        np.add.at(rowsum, pb, np.abs(blocks).sum(1))
    diag[:, np.arange(7), np.arange(7)] = 1.0 + rowsum
    rhs = ((np.arange(7 * nfree) * 31 + 7) % 17 - 8.0).reshape(nfree, 7)
    return pa, pb, np.ascontiguousarray(diag), np.ascontiguousarray(blocks.reshape(-1, 7, 7)), rhs


def residual(pa, pb, diag, blocks, rhs, x):
    """|A x - b| / |b| with a block-sparse product."""
    x = np.asarray(x, np.float64).reshape(-1, 7)
    res = np.einsum("srk,sk->sr", diag, x) - rhs
    if len(pa):
        np.add.at(res, pa, np.einsum("krc,kc->kr", blocks, x[pb]))
        np.add.at(res, pb, np.einsum("krc,kr->kc", blocks, x[pa]))
    return float(np.sqrt((res * res).sum() / (rhs * rhs).sum()))
