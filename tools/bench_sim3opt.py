#!/usr/bin/env python3
"""Timing of the pairwise Sim3 optimizer: 8 loop candidates x 100 matches (a quarter gross mismatches), chi_sq 10, num_iter 10 as
module::loop_detector calls it.  Host clock around the synchronous svgpu_sim3_transform_optimize_batch call and around the same work as
8 svgpu_sim3_transform_optimize calls (median of `reps` after a warm-up), a batch of one for the latency of a single problem, and the
HIP-event time per launch of k_sim3_opt (svgpu_profile_select).  Prints one JSON object."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main(reps=31, warm=5, candidates=8, matches=100):
    from stella_vslam_amd import optimize
    from stella_vslam_amd._lib import lib
    from stella_vslam_amd.feature import Context
    from tests import sim3opt_problems as T
    ctx, L = Context(), lib()
    probs = [T._scene(500 + j, matches, T.pinhole(), T.pinhole(480.0, 482.0, 330.0, 250.0), False, 10, gross=matches // 4) for j in range(candidates)]
    off = (np.arange(candidates + 1) * matches).astype(np.int32)
    cat = lambda k: np.concatenate([p[k] for p in probs])
    arrays = [cat(k) for k in ("obs1", "obs2", "w1", "w2", "pos1", "pos2")]
    sim3 = np.array([p["sim3"] for p in probs])
    view1 = (probs[0]["cam1"], probs[0]["pose1"])
    views2 = [(p["cam2"], p["pose2"]) for p in probs]

    def batch(k=candidates):
        return optimize.sim3_transform_optimize_batch(ctx, view1, views2[:k], off[:k + 1], *[a[:k * matches] for a in arrays], sim3[:k], chi_sq=10.0, fix_scale=False,
                                                      num_iter=10)

    def singles():
        return [optimize.sim3_transform_optimize(ctx, view1, (p["cam2"], p["pose2"]), p["obs1"], p["obs2"], p["w1"], p["w2"], p["pos1"], p["pos2"], p["sim3"],
                                                 chi_sq=10.0, fix_scale=False, num_iter=10) for p in probs]

    def clock(f):
        ts = []
        for r in range(warm + reps):
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warm:
                ts.append((t1 - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    first = batch()
    out = dict(shape=f"{candidates} problems x {matches} matches, num_iter 10", reps=reps, warmup=warm, inliers=[int(v) for v in first["num_inliers"]],
               trials=[int(v) for v in first["lm_trials"].sum(1)])
    out["batch_call_ms"] = clock(batch)
    out["single_calls_ms"] = clock(singles)
    out["batch_of_one_ms"] = clock(lambda: batch(1))
    for name, f in (("k_sim3_opt_batch_ms", batch), ("k_sim3_opt_one_ms", lambda: batch(1))):
        L.svgpu_profile_select(ctx.handle, b"k_sim3_opt")
        for _ in range(reps):
            f()
        ms, n = C.c_double(0), C.c_longlong(0)
        L.svgpu_profile_read_class(ctx.handle, b"k_sim3_opt", C.byref(ms), C.byref(n))
        out[name] = round(ms.value / max(n.value, 1), 4)
        L.svgpu_profile_select(ctx.handle, None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
