#!/usr/bin/env python3
"""Power plane replies against the render of the same request: one JSON line per shape (profiles/power_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around the launches, best of 5 after a warm-up, interleaved:
  a  sp_plan_execute (k_frames: decode, transform, pixel epilogue, image and side outputs)
  b  sp_plan_execute_power on the same capture and width (k_frames_power: one launch, 8 bytes per bin)
  c  b followed by sp_plan_power_to_db on the whole plane, in place (each call under its own event pair, the two times added)
Shapes: BASELINE config 1 (cu8, 2^20 samples, n = 512, width = samples / n), config 2 (cf32, 2^24 samples, n = 1024, width =
samples / n: every sample is looked at) and config 2's capture at a screen-wide 2 048 columns (the sparse picture).
b's store bandwidth is the plane's bytes over b's whole time (decode and transform included).
Usage: tools/power_bench.py [--out FILE] [--reps 5]
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
    spun = False
    for name, fmt, log2s, n, window, width in SHAPES:
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        width = width or samples // n
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        d_img = ctx.alloc(4 * width * n)
        small = {k: ctx.alloc(max(v, 16)) for k, v in (("gauge_mins", width), ("gauge_maxs", width), ("gauge_amps", width),
                                                        ("c_hist", 8 * 256), ("cb_hist", 8000), ("dbfs_minmax", 16))}
        d_plane = ctx.alloc(8 * width * n)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)

        def run(leg):
            if leg == "a":
                plan.execute(d_in, nbytes, width, rgba=d_img, **small)
            else:
                plan.execute_power(d_in, nbytes, width, d_plane)
            ctx.synchronize()
            ms = ctx.last_kernel_ms()
            if leg == "c":
                plan.power_to_db(d_plane, width * n, d_plane)
                ctx.synchronize()
                ms += ctx.last_kernel_ms()
            return ms

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
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width, "kernel_a": plan.kernel_name(nbytes, width),
               "kernel_b": plan.power_kernel_name_for(nbytes, width), "a_render_ms": round(best["a"], 4), "b_power_ms": round(best["b"], 4),
               "c_power_db_ms": round(best["c"], 4), "b_over_a": round(best["b"] / best["a"], 4), "c_over_a": round(best["c"] / best["a"], 4),
               "plane_bytes": 8 * width * n, "b_store_gb_s": round(8 * width * n / (best["b"] * 1e-3) / 1e9, 1), "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in list(small.values()) + [d_img, d_plane, d_in]:
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
