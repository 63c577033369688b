#!/usr/bin/env python3
"""Timing of svgpu_new_landmarks_batch: K = 1, 4, 10 neighbours at 2 000 keypoints a side, 400 BoW nodes.  Host clock around the synchronous
call and, in the same process and run on the same inputs, around the only path that gave these results before: K single matcher calls plus
K single triangulator calls with has_lm1 updated on the host between them (single_device_calls of tests/new_landmarks_problems.py).  100
calls after 20 warm-up calls, median and the 10 % / 90 % quantiles; the outputs are asserted equal first, positions as raw bit patterns.
For information only, the time of the two independent batch calls composed (svgpu_match_for_triangulation_batch, then
svgpu_triangulate_two_views_batch): their RESULTS DIFFER from the loop's wherever a keypoint matches in two neighbours.  Also what the call
reports as issued and, in a run of its own, the HIP-event time per call of every kernel class (svgpu_profile_select("*"); the chain of
k_newlm_init / k_newlm_replay / k_newlm_triangulate launches is the class "k_newlm_chain").  Prints one JSON object."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CENTRES = [(0.35, 0.02, -0.03), (-0.3, 0.05, 0.1), (0.05, -0.4, 0.02), (0.08, 0.0, 0.25), (0.2, 0.2, 0.0), (-0.2, -0.25, 0.05), (0.4, -0.1, 0.1),
           (-0.35, 0.2, -0.05), (0.1, 0.35, 0.1), (-0.1, -0.3, 0.2)]
CLASSES = ("k_bucket_batch", "k_cand_batch", "k_newlm_chain")


def main(reps=100, warm=20, counts=(1, 4, 10), n=2000, nodes=400):
    from stella_vslam_amd._lib import lib
    from stella_vslam_amd.feature import Context
    from tests import new_landmarks_problems as NP
    ctx = Context()
    out = dict(shape=f"{n} keypoints a side, {nodes} nodes", reps=reps, warmup=warm, cases=[])

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
        extra = n - (n * 17 // 20)
        p = NP.make(50 + K, n * 17 // 20, CENTRES[:K], extra1=extra - 40, shadows=40, extras2=[extra] * K, n_nodes=nodes, taken_frac=0.1, name=f"bench{K}")
        assert len(p["side1"]["desc"]) == n and all(len(s["desc"]) == n for s in p["side2"])

        def batch():
            return NP.run_device(ctx, p)

        def singles():
            return NP.single_device_calls(ctx, p)

        def composed():
            return NP.composed_batches(ctx, p)

        got, ref = batch(), singles()
        for key in ("matched_2_in_1", "status", "num_matches", "num_accepted", "created_by"):
            assert np.array_equal(got[key], ref[key]), key
        assert got["pos_w"].tobytes() == ref["pos_w"].tobytes()
        indep = composed()
        case = dict(neighbours=K, num_matches=got["num_matches"].tolist(), num_accepted=got["num_accepted"].tolist(), **got["stats"],
                    composed_batches_accept=[int(v) for v in indep[3]], composed_batches_results_differ=bool(not np.array_equal(indep[0], got["matched_2_in_1"])))
        case["batch_call_ms"], case["batch_p10_ms"], case["batch_p90_ms"] = clock(batch)
        case.update(batch()["stats"])  # (of a call on a warm arena: the first call of a size repeats pass 0 when the arena regrows for the lists)
        case["single_calls_ms"], case["single_p10_ms"], case["single_p90_ms"] = clock(singles)
        case["composed_batches_ms"], case["composed_p10_ms"], case["composed_p90_ms"] = clock(composed)
        spread = (case["batch_p90_ms"] - case["batch_p10_ms"]) + (case["single_p90_ms"] - case["single_p10_ms"])
        case["ahead_by_ms"], case["spreads_added_ms"] = round(case["single_calls_ms"] - case["batch_call_ms"], 4), round(spread, 4)
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
