#!/usr/bin/env python3
"""Timing of svgpu_loop_sim3_batch: K = 1, 4, 10 loop candidates at 2 000 keypoints per keyframe (40 prior matches each, margin 7.5).  Host
clock around the synchronous call and, in the same run with the same inputs, around the same work as the chain of the existing single
calls per candidate -- the scale in numpy, svgpu_match_keyframes_mutually, the gather on the host, svgpu_sim3_transform_optimize
(compose_single_calls of tests/loop_sim3_problems.py): 100 calls after 20 warm-up calls, median and the 10 % / 90 % quantiles.  Also the
launches, copies and synchronisations the batch call reports, and the HIP-event time per call of every kernel class (svgpu_profile_select).  Prints one JSON object."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main(reps=100, warm=20, counts=(1, 4, 10), n=2000):
    from stella_vslam_amd import loop_detector
    from stella_vslam_amd.feature import Context
    from tests import loop_sim3_problems as LP
    import ctypes as C
    from stella_vslam_amd._lib import lib
    KEYS, _cam = LP.KEYS, LP.oracle_camera
    CLASSES = ("k_loop_scale", "k_loop_bin", "k_loop_reproject", "k_loop_walk", "k_cand_batch", "k_loop_edges", "k_sim3_opt")
    ctx = Context()
    out = dict(shape=f"{n} keypoints per keyframe, 40 prior matches per candidate", reps=reps, warmup=warm, cases=[])

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
        p = LP.make(f"bench{K}", [LP.cand(n2=n, n_shared=1400, n_prior=40, seed=s) for s in range(K)], n1=n, seed=40)
        cam1, cams2 = _cam(p["cam1"]), [_cam(c) for c in p["cam2"]]
        kw = {k: p[k] for k in KEYS}
        backend = LP.device_backend(ctx, _cam)

        def batch():
            return loop_detector.validate_sim3_batch(ctx, cam1, cams2, want_stats=True, **kw)

        def singles():
            return LP.compose_single_calls(p, backend)

        got, ref = batch(), singles()
        assert LP.same(got, ref) == []
        case = dict(candidates=K, accepted=int((got["status"] == 0).sum()), num_mutual=got["num_mutual"].tolist(), num_inliers=got["num_inliers"].tolist(),
                    launches=got["stats"][0], copies=got["stats"][1], synchronisations=got["stats"][2])
        case["batch_call_ms"], case["batch_p10_ms"], case["batch_p90_ms"] = clock(batch)
        case["single_calls_ms"], case["single_p10_ms"], case["single_p90_ms"] = clock(singles)
        # HIP events around every kernel class of the call, in a run of its own: mean device time per call, microseconds
        L = lib()
        L.svgpu_profile_select(ctx.handle, b"*")
        for _ in range(20):
            batch()
        case["kernel_us_per_call"] = {}
        for name in CLASSES:
            ms, cnt = C.c_double(0), C.c_longlong(0)
            L.svgpu_profile_read_class(ctx.handle, name.encode(), C.byref(ms), C.byref(cnt))
            case["kernel_us_per_call"][name] = round(ms.value * 1e3 / 20, 2)
        L.svgpu_profile_select(ctx.handle, None)
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
