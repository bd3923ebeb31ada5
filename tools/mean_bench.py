#!/usr/bin/env python3
"""The exact mean-power trace against the power plane of the same request: one JSON line per shape (profiles/mean_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  a  sp_plan_execute_power into a resident plane (k_frames_power: one launch, 8 bytes per bin)
  b  sp_plan_execute_mean with the default window (the same frame loop block by block into the window, k_mean_accumulate behind each
     block, the workspace's clear and k_mean_finish)
  c  sp_power_mean alone on the resident plane of leg a (clear, k_mean_accumulate over the whole plane, k_mean_finish)
Shapes: cf32, n = 1024, 2^24 samples at width 16 384 (every sample is looked at) and at a screen-wide 2 048; cu8, n = 512, 2^24 samples
at width 4 096.  b / a is what the mean costs over the plane it never holds; c is reported as plane bytes per second.
Usage: tools/mean_bench.py [--out FILE] [--reps 5]
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

SHAPES = (("cf32_w16384", "CF32", 24, 1024, "blackmanHarris", 16384), ("cf32_w2048", "CF32", 24, 1024, "blackmanHarris", 2048),
          ("cu8_w4096", "CU8", 24, 512, "hann", 4096))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = load_package()
    ctx = pkg.Context(0)
    ctx.enable_timing(True)
    lut = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)
    lines = []
    spun = False
    for name, fmt, log2s, n, window, width in SHAPES:
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        d_plane = ctx.alloc(8 * width * n)
        d_mean = ctx.alloc(2 * 8 * n)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)

        def run(leg):
            if leg == "a":
                plan.execute_power(d_in, nbytes, width, d_plane)
            elif leg == "b":
                plan.execute_mean(d_in, nbytes, width, d_mean)
            else:
                ctx.power_mean(d_plane, n, width, d_mean + 8 * n)
            ctx.synchronize()
            return ctx.last_kernel_ms()

        t_end = time.time() + (0.0 if spun else 0.5)   # one spin-up: the clocks ramp over the first few hundred milliseconds
        while time.time() < t_end:
            run("a")
        spun = True
        best = {}
        for leg in "abc":
            run(leg)                                   # warm-up of this leg
        for _ in range(args.reps):                     # the legs interleaved: a drift of the box hits all alike
            for leg in "abc":
                best[leg] = min(best.get(leg, 1e30), run(leg))
        means = ctx.download(d_mean, 2 * 8 * n, np.uint64)
        plane_bytes = 8 * width * n
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width,
               "kernel_a": plan.power_kernel_name_for(nbytes, width), "kernel_b": plan.mean_kernel_name_for(nbytes, width),
               "a_power_ms": round(best["a"], 4), "b_mean_ms": round(best["b"], 4), "c_power_mean_ms": round(best["c"], 4),
               "b_over_a": round(best["b"] / best["a"], 4), "plane_bytes": plane_bytes,
               "c_plane_gb_s": round(plane_bytes / (best["c"] * 1e-3) / 1e9, 1), "b_equals_c": bool((means[:n] == means[n:]).all()),
               "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_plane, d_mean, d_in):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
