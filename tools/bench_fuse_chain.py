#!/usr/bin/env python3
"""Timing of svgpu_fuse_landmarks_batch: K = 1, 4, 10, 20 targets at 2 000 keypoints a keyframe and 1 000 landmarks on the current keyframe.
Host clock around the synchronous call and, in the same process and run on the same inputs, around the only path that gave these results
before: the chain of svgpu_fuse_detect_duplication / svgpu_landmarks_compute_descriptor / svgpu_landmarks_update_geometry calls with the
host update between them (tests/fuse_chain_problems.chain over the device calls; its bookkeeping is numpy, which the yardstick includes).
100 calls after 20 warm-up calls (FUSE_BENCH_REPS / FUSE_BENCH_WARM override), median and the 10 % / 90 % quantiles; the outputs are
asserted equal first, floats as raw bit patterns.  Also what the call reports as issued.  Prints one JSON object per K, then all of them."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main(counts=(1, 4, 10, 20), n_points=1000, n_clutter=1000):
    from oracle import oracle as O
    from stella_vslam_amd.feature import Context
    from tests import fuse_chain_problems as F
    from tests import test_gpu_fuse_chain as G
    reps, warm = int(os.environ.get("FUSE_BENCH_REPS", 100)), int(os.environ.get("FUSE_BENCH_WARM", 20))
    ctx = Context()
    out = dict(shape=f"{n_points + n_clutter} keypoints a keyframe, {n_points} landmarks on the current keyframe", reps=reps, warmup=warm, cases=[])

    def clock(f):
        ts = []
        for r in range(warm + reps):
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warm:
                ts.append((t1 - t0) * 1e3)
        return [round(float(v), 4) for v in np.quantile(ts, [0.5, 0.1, 0.9])]

    for K in counts:
        p = F.initial_refresh(F.build(name=f"bench{K}", K=K, n_points=n_points, n_clutter=n_clutter, seed=100 + K), O.landmarks_compute_descriptor,
                              O.landmarks_update_geometry)
        cams = G.gpu_cams(p, ctx)
        got, ref = G.batch(p, ctx, cams), G.single_chain(p, ctx, cams)
        assert got["status"] == 0
        F.assert_same(p, got, ref, "bench")
        case = dict(targets=K, num_fused=got["num_fused"].tolist(), events=np.bincount(got["event"], minlength=6).tolist(), **got["stats"])
        case["batch_call_ms"], case["batch_p10_ms"], case["batch_p90_ms"] = clock(lambda: G.batch(p, ctx, cams))
        case.update(G.batch(p, ctx, cams)["stats"])  # (of a call on a warm arena)
        case["single_calls_ms"], case["single_p10_ms"], case["single_p90_ms"] = clock(lambda: G.single_chain(p, ctx, cams))
        spread = (case["batch_p90_ms"] - case["batch_p10_ms"]) + (case["single_p90_ms"] - case["single_p10_ms"])
        case["ahead_by_ms"], case["spreads_added_ms"] = round(case["single_calls_ms"] - case["batch_call_ms"], 4), round(spread, 4)
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
