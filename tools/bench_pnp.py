#!/usr/bin/env python3
"""Timing of the PnP entry points: 10 candidate keyframes x 150 matches (20 % outliers) x 30 RANSAC iterations, recompute on.
Host clock around the synchronous svgpu_pnp_ransac_batch call and around the same work as 10 svgpu_pnp_ransac calls (median of `reps`
after a warm-up), and the HIP-event time per launch of the three kernel classes (svgpu_profile_select).  Prints one JSON object."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main(reps=31, warm=5):
    from stella_vslam_amd import solve
    from stella_vslam_amd._lib import lib
    from stella_vslam_amd.feature import Context
    from tests import pnp_problems as T
    ctx, L = Context(), lib()
    probs = [T.planted(300 + j, 150, T.KINDS[j % 3], outliers=0.2) for j in range(10)]
    for j, p in enumerate(probs):
        p["samples"] = T.draw_samples(np.random.default_rng(700 + j), 150, 30)
    off, brg, pw, octv = T.concatenate(probs)
    smp, sf = np.stack([p["samples"] for p in probs]), T.orb_scale_factors()

    def batch():
        return solve.pnp_ransac_batch(ctx, off, brg, pw, octv, sf, smp, 10, True, 10)

    def singles():
        return [solve.pnp_ransac(ctx, p["bearings"], p["pos_w"], p["octaves"], sf, p["samples"], 10, True, 10) for p in probs]

    def clock(f):
        ts = []
        for r in range(warm + reps):
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warm:
                ts.append((t1 - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    out = dict(shape="10 problems x 150 matches x 30 iterations, recompute", reps=reps, warmup=warm, valid=int(batch()["valid"].sum()))
    out["batch_call_ms"] = clock(batch)
    out["single_calls_ms"] = clock(singles)
    L.svgpu_profile_select(ctx.handle, b"*")
    for _ in range(reps):
        batch()
    for name in ("k_pnp_ransac", "k_pnp_select", "k_pnp_pose"):
        ms, n = C.c_double(0), C.c_longlong(0)
        L.svgpu_profile_read_class(ctx.handle, name.encode(), C.byref(ms), C.byref(n))
        out[name + "_ms"] = round(ms.value / max(n.value, 1), 4)
    L.svgpu_profile_select(ctx.handle, None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
