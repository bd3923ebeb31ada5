#!/usr/bin/env python3
"""The persistence spectrum against the indexed render it is counted from: one JSON line per shape (profiles/density_bench.jsonl).

Device-resident legs in one process behind one spin-up, HIP events around the launches (the context's event pair), best of --reps
after a warm-up, interleaved:
  a       sp_plan_execute_index (k_frames_index): the yardstick     a2  the same leg again: |a2 / a - 1| is the run's noise margin
  b       sp_plan_execute_density: a's render into the context's workspace, the clear and the count
  c       sp_density_from_index alone on a's image                  c_flat  the same on an all-zero image of the same size
Shapes: BASELINE config 1 (cu8, 2^20 samples, n = 512), config 2 (cf32, 2^24 samples, n = 1024) and config 2's capture at 2 048
columns, each in both layouts (a and b render the layout, c counts it).
Usage: tools/density_bench.py [--out FILE] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SHAPES = (("cfg1", "CU8", 20, 512, "hann", None), ("cfg2", "CF32", 24, 1024, "blackmanHarris", None),
          ("cfg2_w2048", "CF32", 24, 1024, "blackmanHarris", 2048))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = load_package()
    ctx = pkg.Context(0)
    ctx.enable_timing(True)
    lut = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 3) & 255], axis=1).astype(np.uint8)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    spun = False
    for name, fmt, log2s, n, window, width in SHAPES:
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        width = width or samples // n
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        d_ix, d_flat = ctx.alloc(width * n), ctx.alloc(width * n)
        ctx.memset(d_flat, 0, width * n)
        d_den, d_den2 = ctx.alloc(4 * n * 256), ctx.alloc(4 * n * 256)
        small = {k: ctx.alloc(max(v, 16)) for k, v in (("gauge_mins", width), ("gauge_maxs", width), ("gauge_amps", width),
                                                        ("c_hist", 8 * 256), ("cb_hist", 8000), ("dbfs_minmax", 16))}
        for wf in (False, True):
            plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut, False, wf)

            def run(leg):
                if leg in ("a", "a2"):
                    plan.execute_index(d_in, nbytes, width, index=d_ix, **small)
                elif leg == "b":
                    plan.execute_density(d_in, nbytes, width, d_den)
                elif leg == "c":
                    ctx.density_from_index(d_ix, n, width, wf, 256, d_den2)
                else:
                    ctx.density_from_index(d_flat, n, width, wf, 256, d_den2)
                ctx.synchronize()
                return ctx.last_kernel_ms()

            t_end = time.time() + (0.0 if spun else 0.5)   # one spin-up: the clocks ramp over the first few hundred milliseconds
            while time.time() < t_end:
                run("a")
            spun = True
            legs = ("a", "b", "c", "c_flat", "a2")
            best = {}
            same = None
            for leg in legs:
                run(leg)                                   # warm-up of this leg (the workspace)
                if leg == "c":                             # b's counts are c's of a's image
                    same = bool(np.array_equal(ctx.download(d_den, 4 * n * 256), ctx.download(d_den2, 4 * n * 256)))
            for _ in range(args.reps):                     # the legs interleaved: a drift of the box hits all alike
                for leg in legs:
                    best[leg] = min(best.get(leg, 1e30), run(leg))
            launch = pkg.Library.get().debug_density_launch(n, width, wf)
            emit({"shape": name + ("_wf" if wf else ""), "format": fmt, "n": n, "samples": samples, "width": width, "waterfall": wf,
                  "kernel_a": plan.index_kernel_name_for(nbytes, width), "count_workgroups": launch["workgroups"],
                  "a_index_ms": round(best["a"], 4), "b_density_ms": round(best["b"], 4), "c_count_ms": round(best["c"], 4),
                  "c_flat_ms": round(best["c_flat"], 4), "b_over_a": round(best["b"] / best["a"], 4),
                  "c_over_a": round(best["c"] / best["a"], 4), "c_flat_over_c": round(best["c_flat"] / best["c"], 4),
                  "b_minus_a_minus_c_ms": round(best["b"] - best["a"] - best["c"], 4), "count_GBps": round(width * n / best["c"] / 1e6, 1),
                  "noise_a2_over_a": round(best["a2"] / best["a"], 4), "b_equals_c": same, "reps": args.reps})
            plan.close()
        for p in list(small.values()) + [d_ix, d_flat, d_den, d_den2, d_in]:
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
