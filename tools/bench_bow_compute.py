#!/usr/bin/env python3
"""Times of registering B keyframes of 2 000 descriptors in the BoW database (MI355X): the one call
data::hip::bow_database::add_keyframes(keyframes, vocabulary) -- svgpu_bow_compute_batch with its registration path -- against the only
path that gave these results before it: B x (compute_bow: one transform call and the C++ host accumulation; add_keyframe: one
svgpu_bowdb_add).  Both run in the same process (host/test_bow_compute --bench), outputs are asserted equal first; host clock around the
synchronous calls, median and p10 - p90 after warm-up; per-kernel-class HIP-event times from a run of their own.  Prints the markdown
rows of DESIGN section 21 and the smallest B at which the batch is ahead by more than the two spreads added.

  python tools/bench_bow_compute.py [--frames 1 16 256 2000] [--descriptors 2000] [--calls 50]
"""
import argparse
import json
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
EXE = ROOT / "stella_vslam_amd" / "host" / "test_bow_compute"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16, 256, 2000])
    ap.add_argument("--descriptors", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    if not EXE.exists():
        raise SystemExit(f"{EXE} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    rows, ahead_from = [], None
    for b in a.frames:
        r = subprocess.run([str(EXE), "--bench", str(b), str(a.descriptors), str(a.calls)], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"B = {b}: the batch and the loop disagree, or the run failed\n{r.stdout}{r.stderr}")
        j = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(j), flush=True)
        rows.append(j)
    print("\n| B | one call ms (p10 - p90) | B x (compute_bow + add_keyframe) ms (p10 - p90) | ahead by ms (spreads added) | ratio | descent / order / sums us |")
    print("|---|---|---|---|---|---|")
    for j in rows:
        (b0, b1, b2), (l0, l1, l2) = j["batch_ms"], j["loop_ms"]
        spreads = (b2 - b0) + (l2 - l0)
        if ahead_from is None and l1 - b1 > spreads:
            ahead_from = j["frames"]
        print(f"| {j['frames']} | {b1:.3f} ({b0:.3f} - {b2:.3f}) | {l1:.3f} ({l0:.3f} - {l2:.3f}) | {l1 - b1:.3f} ({spreads:.3f}) | {l1 / b1:.2f} x | "
              f"{j['descend_us']:.0f} / {j['sort_us']:.0f} / {j['emit_us']:.0f} |")
    print(f"\nthe batch call is ahead by more than the two spreads added from B = {ahead_from}" if ahead_from is not None
          else "\nthe batch call is ahead of the loop at none of these B")


if __name__ == "__main__":
    main()
