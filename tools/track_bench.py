#!/usr/bin/env python3
"""The peak track against the power plane and the band-power series of the same request: one JSON line per shape
(profiles/track_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  a   sp_plan_execute_power into a resident plane (k_frames_power: one launch, 8 bytes per bin)
  b   sp_plan_execute_track of one full band with the default window (the same frame loop block by block into the window, k_track_max
      behind each block)
  c1  sp_power_tracks alone on the resident plane of leg a, one full band [0, n) (k_track_max: one launch)
  c8  ... eight bands of n/8 rows (the same bytes, eight times the workgroups)
  d   sp_power_bands of [0, n) on the same plane: the band sum's code reading the same bytes (k_band_sum<0>) - the yardstick for c1
Shapes: tools/mean_bench.py's.  c1 / d is reported; c1 as plane bytes per second.
Usage: tools/track_bench.py [--out FILE] [--reps 5]
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
LEGS = ("a", "b", "c1", "c8", "d")


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
        d_row = ctx.alloc(10 * 4 * width)              # b, c1, then c8's eight tracks
        d_peak = ctx.alloc(10 * 8 * width)
        d_band = ctx.alloc(8 * width)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        full, eighths = [(0, n)], [(k * n // 8, (k + 1) * n // 8) for k in range(8)]

        def run(leg):
            if leg == "a":
                plan.execute_power(d_in, nbytes, width, d_plane)
            elif leg == "b":
                plan.execute_track(d_in, nbytes, width, full, d_row, d_peak)
            elif leg == "c1":
                ctx.power_tracks(d_plane, n, width, full, d_row + 4 * width, d_peak + 8 * width)
            elif leg == "c8":
                ctx.power_tracks(d_plane, n, width, eighths, d_row + 2 * 4 * width, d_peak + 2 * 8 * width)
            else:
                ctx.power_bands(d_plane, n, width, full, d_band)
            ctx.synchronize()
            return ctx.last_kernel_ms()

        t_end = time.time() + (0.0 if spun else 0.5)   # one spin-up: the clocks ramp over the first few hundred milliseconds
        while time.time() < t_end:
            run("a")
        spun = True
        best = {}
        for leg in LEGS:
            run(leg)                                   # warm-up of this leg
        for _ in range(args.reps):                     # the legs interleaved: a drift of the box hits all alike
            for leg in LEGS:
                best[leg] = min(best.get(leg, 1e30), run(leg))
        peaks = ctx.download(d_peak, 2 * 8 * width, np.uint64)
        rows = ctx.download(d_row, 2 * 4 * width, np.int32)
        plane_bytes = 8 * width * n
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width,
               "kernel_a": plan.power_kernel_name_for(nbytes, width), "kernel_b": plan.track_kernel_name_for(nbytes, width),
               "a_power_ms": round(best["a"], 4), "b_track_ms": round(best["b"], 4), "c1_power_tracks_full_ms": round(best["c1"], 4),
               "c8_power_tracks_eighths_ms": round(best["c8"], 4), "d_power_bands_ms": round(best["d"], 4),
               "b_over_a": round(best["b"] / best["a"], 4), "c1_over_d": round(best["c1"] / best["d"], 4),
               "c8_over_c1": round(best["c8"] / best["c1"], 4), "plane_bytes": plane_bytes,
               "c1_plane_gb_s": round(plane_bytes / (best["c1"] * 1e-3) / 1e9, 1), "d_plane_gb_s": round(plane_bytes / (best["d"] * 1e-3) / 1e9, 1),
               "b_equals_c1": bool((peaks[:width] == peaks[width:]).all() and (rows[:width] == rows[width:]).all()),
               "distinct_rows": int(len(np.unique(rows[:width]))), "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_plane, d_band, d_row, d_peak, d_in):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
