#!/usr/bin/env python3
"""Timing of svgpu_pose_graph_optimize on chains with windowed covisibility and one loop (class e of tests/posegraph_problems.py) of
`--sizes` vertices: host clock around the synchronous call (median of `--reps` after `--warm` warm-up calls) and the HIP-event time
of the kernel classes per call (svgpu_profile_select): linearise, assemble, solve (preconditioner + PCG) and trial (update, chi2,
decision), with the LM and PCG iteration counts.  Prints one JSON object per size.  --solver envelope times the direct solver
(svgpu_pose_graph_optimize_ex) instead, with its two kernel classes; --solver both prints one object per size and solver, the PCG first."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300,2000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--fix-scale", type=int, default=0)
    ap.add_argument("--solver", choices=["pcg", "envelope", "both"], default="pcg")
    ap.add_argument("--profile", type=int, default=1, help="0: skip the extra call that collects the per-class kernel times")
    a = ap.parse_args()
    from stella_vslam_amd import optimize
    from stella_vslam_amd._lib import lib
    from stella_vslam_amd.feature import Context
    from tests import posegraph_problems as T
    ctx, L = Context(), lib()
    for n in (int(s) for s in a.sizes.split(",")):
        for solver in (["pcg", "envelope"] if a.solver == "both" else [a.solver]):
            p = T._class_e(7, bool(a.fix_scale), n=n)
            extra = {} if solver == "pcg" else dict(solver=solver)

            def call():
                return optimize.pose_graph_optimize(ctx, p["sim3"], p["fixed"], p["e1"], p["e2"], p["meas"], fix_scale=p["fix_scale"], **extra)

            ts, res = [], None
            for r in range(a.warm + a.reps):
                t0 = time.perf_counter()
                res = call()
                t1 = time.perf_counter()
                if r >= a.warm:
                    ts.append((t1 - t0) * 1e3)
            out = dict(shape=f"chain of {n}, window 3, one loop, 3 fixed", vertices=n, edges=len(p["e1"]), fix_scale=int(p["fix_scale"]), reps=a.reps, warmup=a.warm,
                       call_ms=round(float(np.median(ts)), 3), lm_iterations=res["lm_iterations"], lm_trials=res["lm_trials"],
                       pcg_iterations=res["pcg_iterations"], pcg_capped=res["pcg_capped"], initial_chi2=res["initial_chi2"], final_chi2=res["final_chi2"])
            classes = ("k_pg_linearize", "k_pg_assemble", "k_pg_solve", "k_pg_trial")
            if solver != "pcg":
                out.update(solver=solver, ordering=res["ordering"], envelope_blocks=res["envelope_blocks"], max_column_rows=res["max_column_rows"],
                           failed_solves=res["failed_solves"])
                classes = ("k_pg_linearize", "k_pg_assemble", "k_pg_env_assemble", "k_pg_env_factor_solve", "k_pg_trial")
            if a.profile:
                L.svgpu_profile_select(ctx.handle, b"*")
                call()
            for name in classes if a.profile else ():
                ms, cnt = C.c_double(0), C.c_longlong(0)
                L.svgpu_profile_read_class(ctx.handle, name.encode(), C.byref(ms), C.byref(cnt))
                out[name + "_ms_per_call"] = round(ms.value, 4)
            L.svgpu_profile_select(ctx.handle, None)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
