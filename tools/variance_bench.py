#!/usr/bin/env python3
"""The exact variance sums against the exact mean of the same plane: one JSON line per shape, then one per finish size
(profiles/variance_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  pm      sp_power_mean on a resident plane (a memset, k_mean_accumulate, k_mean_finish) - the yardstick of pv
  pv      sp_power_variance on the same plane (a memset, k_variance_accumulate, k_variance_finish)
  em      sp_plan_execute_mean with the default window - the yardstick of ev
  ev      sp_plan_execute_variance (the same frame loop block by block, the accumulation behind each block)
Shapes: tools/band_bench.py's.  Every ratio to its yardstick is reported, and pm and pv as plane bytes per second.
The finish: sp_power_variance and sp_power_mean over 32 frames of noise-like power at n = 1024 and n = 8192 - one workgroup piece per
band, so the call is the clear, a minimal accumulation and the finish: an upper bound of the finish's time, a line of its own.
Usage: tools/variance_bench.py [--out FILE] [--reps 5]
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
LEGS = ("pm", "pv", "em", "ev")
FINISH = ((1024, 32), (8192, 32))


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
        d_mean = ctx.alloc(8 * n)
        d_var = ctx.alloc(3 * 8 * n)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        plan.execute_power(d_in, nbytes, width, d_plane)
        ctx.synchronize()

        def run(leg):
            if leg == "pm":
                ctx.power_mean(d_plane, n, width, d_mean)
            elif leg == "pv":
                ctx.power_variance(d_plane, n, width, d_var)
            elif leg == "em":
                plan.execute_mean(d_in, nbytes, width, d_mean)
            else:
                plan.execute_variance(d_in, nbytes, width, d_var)
            ctx.synchronize()
            return ctx.last_kernel_ms()

        t_end = time.time() + (0.0 if spun else 0.5)   # one spin-up: the clocks ramp over the first few hundred milliseconds
        while time.time() < t_end:
            run("pm")
        spun = True
        best = {}
        for leg in LEGS:
            run(leg)                                   # warm-up of this leg
        for _ in range(args.reps):                     # the legs interleaved: a drift of the box hits all alike
            for leg in LEGS:
                best[leg] = min(best.get(leg, 1e30), run(leg))
        # out[0] / width of the last variance leg is the mean of the last mean leg, bit for bit
        s1 = ctx.download(d_var, 8 * n, np.float64)
        same = bool(((s1 / np.float64(width)).view(np.uint64) == ctx.download(d_mean, 8 * n, np.uint64)).all())
        plane_bytes = 8 * width * n
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width,
               "kernel_ev": plan.variance_kernel_name_for(nbytes, width), "plane_bytes": plane_bytes, "reps": args.reps,
               "launch": list(pkg.binding.debug_variance_launch(n, width, 256)), "sum_over_width_equals_mean": same}
        for leg in LEGS:
            rec[leg + "_ms"] = round(best[leg], 4)
        rec["pv_over_pm"] = round(best["pv"] / best["pm"], 3)
        rec["ev_over_em"] = round(best["ev"] / best["em"], 3)
        rec["pm_plane_gb_s"] = round(plane_bytes / (best["pm"] * 1e-3) / 1e9, 1)
        rec["pv_plane_gb_s"] = round(plane_bytes / (best["pv"] * 1e-3) / 1e9, 1)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_plane, d_mean, d_var, d_in):
            ctx.free(p)

    rng = np.random.default_rng(25)
    for n, frames in FINISH:
        plane = rng.exponential(1e-3, (frames, n))     # noise-like power: a few neighbouring cells per row
        d_plane, d_mean, d_var = ctx.alloc(plane.nbytes), ctx.alloc(8 * n), ctx.alloc(3 * 8 * n)
        ctx.upload(d_plane, plane.view(np.uint8).reshape(-1))
        best = {}
        for rep in range(args.reps + 1):               # (the first round is the warm-up)
            for leg in ("pm", "pv"):
                if leg == "pm":
                    ctx.power_mean(d_plane, n, frames, d_mean)
                else:
                    ctx.power_variance(d_plane, n, frames, d_var)
                ctx.synchronize()
                if rep:
                    best[leg] = min(best.get(leg, 1e30), ctx.last_kernel_ms())
        rec = {"shape": "finish_n%d" % n, "n": n, "frames": frames, "what": "clear + one piece per band + finish",
               "pm_ms": round(best["pm"], 4), "pv_ms": round(best["pv"], 4), "pv_over_pm": round(best["pv"] / best["pm"], 3)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        for p in (d_plane, d_mean, d_var):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
