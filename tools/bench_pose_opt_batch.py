#!/usr/bin/env python3
"""Timing of the batched pose optimizer: K = 1, 4, 16, 64 candidates of one frame, 300 entries each of which `select` keeps 150 (as the
inliers of a PnP RANSAC would).  Host clock around the synchronous svgpu_pose_optimize_batch call and, in the same run, around the same work
as K svgpu_pose_optimize calls with the compaction on the host (200 calls after 20 warm-up calls, median and the 10 % / 90 % quantiles),
and the HIP-event time per launch of k_pose_opt_batch (svgpu_profile_select).  Prints one JSON object."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main(reps=200, warm=20, counts=(1, 4, 16, 64), entries=300):
    from stella_vslam_amd import optimize
    from stella_vslam_amd._lib import lib
    from stella_vslam_amd.feature import Context
    from tests.test_oracle_ba import _pose_problem
    ctx, L = Context(), lib()
    po = optimize.pose_optimizer(ctx=ctx)
    probs = []
    for j in range(max(counts)):
        pr = _pose_problem(900 + j, n=entries + 40)
        assert len(pr["pos_w"]) >= entries
        probs.append({k: (v[:entries] if k in ("pos_w", "uvr", "inv_sigma_sq", "huber") else v) for k, v in pr.items()})
    select = np.zeros(entries, np.uint8)
    select[::2] = 1
    keep = select != 0
    out = dict(shape=f"{entries} entries per candidate, {int(keep.sum())} selected, trials 2 / 2 / 10", reps=reps, warmup=warm, cases=[])

    def clock(f):
        ts = []
        for r in range(warm + reps):
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warm:
                ts.append((t1 - t0) * 1e3)
        q = np.quantile(ts, [0.5, 0.1, 0.9])
        return [round(float(v), 4) for v in q]

    for K in counts:
        ps = probs[:K]
        off = (np.arange(K + 1) * entries).astype(np.int32)
        cat = lambda k: np.concatenate([p[k] for p in ps])
        poses, pw, uv, w, hb, sel = np.stack([p["pose_cw"] for p in ps]), cat("pos_w"), cat("uvr"), cat("inv_sigma_sq"), cat("huber"), np.tile(select, K)
        intr = ps[0]["intr"]

        def batch():
            return po.optimize_batch_flat(poses, off, pw, uv, w, hb, intr, select=sel)

        def singles():
            return [po.optimize_flat(p["pose_cw"], p["pos_w"][keep], p["uvr"][keep], p["inv_sigma_sq"][keep], p["huber"][keep], intr) for p in ps]

        nv, pose, _, it = batch()
        ref = singles()
        assert all(nv[k] == ref[k][0] and pose[k].tobytes() == ref[k][1].tobytes() for k in range(K))
        case = dict(candidates=K, lm_iterations=int(it.sum()))
        case["batch_call_ms"], case["batch_p10_ms"], case["batch_p90_ms"] = clock(batch)
        case["single_calls_ms"], case["single_p10_ms"], case["single_p90_ms"] = clock(singles)
        L.svgpu_profile_select(ctx.handle, b"k_pose_opt_batch")
        for _ in range(reps):
            batch()
        ms, n = C.c_double(0), C.c_longlong(0)
        L.svgpu_profile_read_class(ctx.handle, b"k_pose_opt_batch", C.byref(ms), C.byref(n))
        L.svgpu_profile_select(ctx.handle, None)
        case["k_pose_opt_batch_ms"] = round(ms.value / max(n.value, 1), 4)
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
