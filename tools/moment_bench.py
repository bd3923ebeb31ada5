#!/usr/bin/env python3
"""The exact spectral moments against the exact band-power series of the same plane: one JSON line per shape
(profiles/moment_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  y1      sp_power_bands on a resident plane, one full band [0, n) (k_band_sum<0>: one launch) - the yardstick of m*_1
  y8      ... eight bands of n/8 rows - the yardstick of m*_8
  m0_1, m1_1, m2_1   sp_power_moments at the orders 0, 1, 2 on the same plane, one full band (k_band_sum<order>: one launch; order 0 is y1's kernel)
  m0_8, m1_8, m2_8   ... eight bands of n/8 rows
  eb      sp_plan_execute_bandpower of one full band with the default window - the yardstick of e2
  e2      sp_plan_execute_moments at order 2 of one full band (the same frame loop block by block, k_band_sum<2> behind each block)
Shapes: tools/band_bench.py's.  Every ratio to its yardstick is reported, and m*_1 as plane bytes per second.
Usage: tools/moment_bench.py [--out FILE] [--reps 5]
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
LEGS = ("y1", "y8", "m0_1", "m1_1", "m2_1", "m0_8", "m1_8", "m2_8", "eb", "e2")


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
        d_band = ctx.alloc(8 * 8 * width)              # y1 / y8 / eb
        d_mom = ctx.alloc(3 * 8 * 8 * width)           # every moment leg: up to three moments of eight bands
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        full, eighths = [(0, n)], [(k * n // 8, (k + 1) * n // 8) for k in range(8)]
        plan.execute_power(d_in, nbytes, width, d_plane)
        ctx.synchronize()

        def run(leg):
            if leg == "y1":
                ctx.power_bands(d_plane, n, width, full, d_band)
            elif leg == "y8":
                ctx.power_bands(d_plane, n, width, eighths, d_band)
            elif leg == "eb":
                plan.execute_bandpower(d_in, nbytes, width, full, d_band)
            elif leg == "e2":
                plan.execute_moments(d_in, nbytes, width, full, 2, d_mom)
            else:
                ctx.power_moments(d_plane, n, width, full if leg.endswith("_1") else eighths, int(leg[1]), d_mom)
            ctx.synchronize()
            return ctx.last_kernel_ms()

        t_end = time.time() + (0.0 if spun else 0.5)   # one spin-up: the clocks ramp over the first few hundred milliseconds
        while time.time() < t_end:
            run("y1")
        spun = True
        best = {}
        for leg in LEGS:
            run(leg)                                   # warm-up of this leg
        for _ in range(args.reps):                     # the legs interleaved: a drift of the box hits all alike
            for leg in LEGS:
                best[leg] = min(best.get(leg, 1e30), run(leg))
        # m[0] of the last moment leg (e2, one full band) is the band-power series of the last band leg (eb), bit for bit
        same = bool((ctx.download(d_mom, 8 * width, np.uint64) == ctx.download(d_band, 8 * width, np.uint64)).all())
        plane_bytes = 8 * width * n
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width,
               "kernel_e2": plan.moments_kernel_name_for(nbytes, width), "plane_bytes": plane_bytes, "reps": args.reps,
               "e2_m0_equals_eb": same}
        for leg in LEGS:
            rec[leg + "_ms"] = round(best[leg], 4)
        for order in (0, 1, 2):
            rec["m%d_1_over_y1" % order] = round(best["m%d_1" % order] / best["y1"], 3)
            rec["m%d_8_over_y8" % order] = round(best["m%d_8" % order] / best["y8"], 3)
            rec["m%d_1_plane_gb_s" % order] = round(plane_bytes / (best["m%d_1" % order] * 1e-3) / 1e9, 1)
        rec["y1_plane_gb_s"] = round(plane_bytes / (best["y1"] * 1e-3) / 1e9, 1)
        rec["e2_over_eb"] = round(best["e2"] / best["eb"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_plane, d_band, d_mom, d_in):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
