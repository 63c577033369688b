#!/usr/bin/env python3
"""Timing of the batched bucket matchers: K = 1, 4, 16, 64 partners in two shapes.
  reloc  K 2 000-keypoint keyframes against ONE 2 000-keypoint frame with node ids (side 2 shared, svgpu_bow_match_batch)
  tri    ONE 2 000-keypoint keyframe against K 2 000-keypoint neighbours (side 1 shared, svgpu_match_for_triangulation_batch)
Host clock around the synchronous batch call and, in the same process and run, around the same work as K calls of the existing single
entry point (200 calls after 20 warm-up calls; median and the 10 % / 90 % quantiles), and the HIP-event time of the classes
k_bucket_batch and k_cand_batch per call (svgpu_profile_select).  Prints one JSON object."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N = 2000


def _keyframe(rng, base_desc, base_node, tri):
    """A keyframe that sees 70 % of the base keypoints again (descriptors with a few bits flipped), the rest clutter."""
    n = len(base_desc)
    desc = base_desc.copy()
    flips = rng.integers(0, 256, (n, 12))
    for k in range(12):
        on = rng.uniform(0, 1, n) < 0.5
        desc[np.arange(n)[on], flips[on, k] >> 3] ^= (1 << (flips[on, k] & 7)).astype(np.uint8)
    clutter = rng.uniform(0, 1, n) < 0.3
    desc[clutter] = rng.integers(0, 256, (int(clutter.sum()), 32), dtype=np.uint8)
    perm = rng.permutation(n)
    s = dict(desc=np.ascontiguousarray(desc[perm]), angle=rng.uniform(0, 360, n).astype(np.float32), node=np.ascontiguousarray(base_node[perm]))
    if tri:
        b = rng.normal(0, 0.3, (n, 3)) + np.array([0, 0, 1.0])
        s.update(bearings=b / np.linalg.norm(b, axis=1, keepdims=True), octave=rng.integers(0, 8, n).astype(np.int32),
                 has_lm=(rng.uniform(0, 1, n) < 0.4).astype(np.uint8))
    else:
        s["valid"] = (rng.uniform(0, 1, n) < 0.8).astype(np.uint8)
    return s


def main(reps=200, warm=20, counts=(1, 4, 16, 64)):
    from stella_vslam_amd import match
    from stella_vslam_amd._lib import lib
    from stella_vslam_amd.feature import Context
    ctx, L = Context(), lib()
    rng = np.random.default_rng(5)
    base_desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    base_node = rng.integers(0, 400, N).astype(np.int32)
    out = dict(shape=f"{N} keypoints a side, 400 nodes", reps=reps, warmup=warm, cases=[])

    def clock(f):
        ts = []
        for r in range(warm + reps):
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warm:
                ts.append((t1 - t0) * 1e3)
        return [round(float(v), 4) for v in np.quantile(ts, [0.5, 0.1, 0.9])]

    bt = match.bow_tree(0.75, True, ctx)
    sf = (1.2 ** np.arange(8)).astype(np.float32)
    for shape in ("reloc", "tri"):
        tri = shape == "tri"
        one = _keyframe(rng, base_desc, base_node, tri)
        many = [_keyframe(rng, base_desc, base_node, tri) for _ in range(max(counts))]
        E = np.tile(np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]]), (max(counts), 1, 1))
        epi = np.tile(np.array([1.0, 0, 0]), (max(counts), 1))
        for K in counts:
            ks = many[:K]
            if tri:
                def batch():
                    return match.match_for_triangulation_batch(ctx, 0.8, True, one, ks, E[:K], epi[:K], np.ones(K, np.int32), sf, 0.05)

                def singles():
                    return [match.match_for_triangulation(ctx, 0.8, True, one["desc"], one["angle"], one["octave"], one["bearings"], one["has_lm"], k["desc"],
                                                          k["angle"], k["bearings"], k["has_lm"], E[0], epi[0], 1, sf, 0.05, node1=one["node"], node2=k["node"])
                            for k in ks]
            else:
                frame = {k: v for k, v in one.items() if k != "valid"}  # (the frame: every keypoint is a candidate)

                def batch():
                    return bt.match_batch(ks, frame)

                def singles():
                    return [bt.match(k["desc"], k["angle"], k["valid"], k["node"], one["desc"], one["angle"], one["node"]) for k in ks]
            lists, nums = batch()
            ref = singles()
            assert all(np.array_equal(lists[k], ref[k][0]) and nums[k] == ref[k][1] for k in range(K))
            case = dict(shape=shape, partners=K, matches=int(nums.sum()))
            case["batch_call_ms"], case["batch_p10_ms"], case["batch_p90_ms"] = clock(batch)
            case["single_calls_ms"], case["single_p10_ms"], case["single_p90_ms"] = clock(singles)
            for cls in (b"k_bucket_batch", b"k_cand_batch"):
                L.svgpu_profile_select(ctx.handle, cls)
                for _ in range(50):
                    batch()
                ms, n = C.c_double(0), C.c_longlong(0)
                L.svgpu_profile_read_class(ctx.handle, cls, C.byref(ms), C.byref(n))
                L.svgpu_profile_select(ctx.handle, None)
                case[cls.decode() + "_ms_per_call"] = round(ms.value / 50, 4)
            out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
