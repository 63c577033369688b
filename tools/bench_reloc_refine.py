#!/usr/bin/env python3
"""Timing of svgpu_reloc_refine_batch: K = 1, 4, 16 candidates of one frame of 2 000 keypoints, 300 keyframe entries each, two stages
({10, 3} px, {100, 64} bits).  Host clock around the synchronous call and, in the same run, around the same work as the chain of
svgpu_match_frame_and_keyframe_projection / svgpu_pose_optimize calls per candidate with the gather on the host (compose_single_calls of
tests/reloc_refine_problems.py): 200 calls after 20 warm-up calls, median and the 10 % / 90 % quantiles.  Also the launches, copies and
synchronisations the batch call reports.  Prints one JSON object."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main(reps=200, warm=20, counts=(1, 4, 16), entries=300, nt=2000):
    from oracle import oracle as O
    from stella_vslam_amd import relocalizer
    from stella_vslam_amd.feature import Context
    from tests import reloc_refine_problems as RP
    from tests.test_gpu_reloc_refine import KEYS
    ctx = Context()
    out = dict(shape=f"{nt} keypoints, {entries} entries per candidate, 2 stages", reps=reps, warmup=warm, cases=[])

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
        p = RP.make(f"bench{K}", [RP.cand(n_init=30, n_entries=entries, roll_deg=1.5, seed=s) for s in range(K)], nt=nt, n_lm=1800, seed=40)
        c = p["cam"]
        cam = O.make_camera(c["model"], c["cols"], c["rows"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"], c["focal_x_baseline"])
        kw = {k: p[k] for k in KEYS}
        backend = RP.device_backend(ctx, cam)

        def batch():
            return relocalizer.refine_pose_batch(ctx, cam, want_stats=True, **kw)

        def singles():
            return RP.compose_single_calls(p, backend)

        got, ref = batch(), singles()
        assert RP.same(got, ref) == []
        case = dict(candidates=K, accepted=int((got["status"] == 0).sum()), num_found=got["num_found"].sum(0).tolist(), launches=got["stats"][0],
                    copies=got["stats"][1], synchronisations=got["stats"][2])
        case["batch_call_ms"], case["batch_p10_ms"], case["batch_p90_ms"] = clock(batch)
        case["single_calls_ms"], case["single_p10_ms"], case["single_p90_ms"] = clock(singles)
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
