#!/usr/bin/env python3
"""The keyframe BoW database leg of tools/bench_extra.py (also runnable alone): 1 000 and 5 000 keyframes of about 1 500 words, one query
and a 64-query batch.  Times are HIP events on the context's stream around the whole call (upload, four launches, read-back), median of
`reps` after a warm-up, with the host wall clock of the same calls beside them, and the host transcription of the reference's algorithm
(host/test_bow_database --bench) on the same box.  Prints one JSON object when run alone."""
import ctypes as C
import json
import os
import pathlib
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _events(ctx, f, reps, warm=3):
    from stella_vslam_amd._lib import lib
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p(lib().svgpu_stream(ctx.handle))
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
    ev, wall = [], []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        assert hip.hipEventRecord(a, stream) == 0
        f()
        assert hip.hipEventRecord(b, stream) == 0 and hip.hipEventSynchronize(b) == 0
        t1 = time.perf_counter()
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
        if r >= warm:
            ev.append(ms.value), wall.append((t1 - t0) * 1e3)
    hip.hipEventDestroy(a), hip.hipEventDestroy(b)
    return round(float(np.median(ev)), 4), round(float(np.median(wall)), 4)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def run(ctx, sizes=(1000, 5000), words=1500, batch=64, reps=25, vocab=100000, host=True):
    from stella_vslam_amd import data
    rng = np.random.default_rng(3)
    out = {"host_cpu": cpu_model(), "words_per_keyframe": words, "reps": reps}

    def vec(n, base=None):
        ids = rng.choice(vocab, n, replace=False) if base is None else np.where(rng.uniform(size=n) < 0.8, base, rng.choice(vocab, n))
        ids = np.unique(ids).astype(np.uint32)
        w = rng.uniform(0.05, 1.0, len(ids))
        return ids, w / np.sqrt((w * w).sum())

    queries = [vec(words) for _ in range(batch)]
    for n_kf in sizes:
        db = data.bow_database(ctx, "fbow")
        for i in range(n_kf):
            db.add_keyframe(vec(words, queries[i % batch][0] if i % 100 == 5 else None))
        single = lambda: db.acquire_keyframes(queries[5], 0.0, 0.8)
        many = lambda: db.acquire_keyframes_batch(queries, 0.0, 0.8)
        ev1, wall1 = _events(ctx, single, reps)
        evb, wallb = _events(ctx, many, reps)
        r = {"entries": db.size()[1], "candidates_single": int(len(single()[0])), "single_query_event_ms": ev1, "single_query_wall_ms": wall1,
             f"batch{batch}_event_ms": evb, f"batch{batch}_wall_ms": wallb, f"batch{batch}_per_query_event_ms": round(evb / batch, 4)}
        exe = ROOT / "stella_vslam_amd" / "host" / "test_bow_database"
        if host and exe.exists():
            p = subprocess.run([str(exe), "--bench", str(n_kf), str(words), str(reps)], capture_output=True, text=True, timeout=600)
            if p.returncode == 0:
                r["host_test_program"] = json.loads(p.stdout.strip().splitlines()[-1])
        out[f"keyframes_{n_kf}"] = r
        db.close()
    return out


if __name__ == "__main__":
    from stella_vslam_amd import feature
    quick = "--quick" in sys.argv  # for a profiler run: one size, no host program, few repetitions
    print(json.dumps(run(feature.Context(0), sizes=(5000,), reps=5, host=False) if quick else run(feature.Context(0))))
