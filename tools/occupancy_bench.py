#!/usr/bin/env python3
"""The occupancy counts against the power plane, the peak track and the exact mean of the same request: one JSON line per shape
(profiles/occupancy_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  a        sp_plan_execute_power into a resident plane (k_frames_power: one launch, 8 bytes per bin)
  b        sp_plan_execute_occupancy, one full band and the rows, with the default window (the same frame loop block by block into the
           window, k_occupancy_count behind each block, two memsets in front)
  c_rows   sp_power_occupancy alone on the resident plane of leg a: the rows only
  c_frames ... the frames of one full band [0, n) only
  c_both   ... both
  c_both8  ... both, eight bands of n/8 rows
  t        sp_power_tracks of [0, n) on the same plane (k_track_max: a compare per value, no atomics) - the lower yardstick
  m        sp_power_mean on the same plane (lane-per-row LDS atomics, three stream operations) - the upper yardstick
The thresholds are 1.5 times the plane's mean trace (sp_power_mean's own reply, multiplied on the host).
Shapes: tools/mean_bench.py's.  c_both / t and c_both / m are reported; b and c_both must give identical words.
Usage: tools/occupancy_bench.py [--out FILE] [--reps 5]
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
LEGS = ("a", "b", "c_rows", "c_frames", "c_both", "c_both8", "t", "m")


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
        d_rows = ctx.alloc(5 * 4 * n)                  # b, c_rows, c_both, c_both8, spare
        d_frames = ctx.alloc(12 * 4 * width)           # b, c_frames, c_both, then c_both8's eight
        d_mean, d_thr = ctx.alloc(8 * n), ctx.alloc(8 * n)
        d_row, d_peak = ctx.alloc(4 * width), ctx.alloc(8 * width)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        full, eighths = [(0, n)], [(k * n // 8, (k + 1) * n // 8) for k in range(8)]
        plan.execute_power(d_in, nbytes, width, d_plane)
        ctx.power_mean(d_plane, n, width, d_mean)
        ctx.synchronize()
        thr = 1.5 * ctx.download(d_mean, 8 * n, np.float64)
        ctx.upload(d_thr, thr.view(np.uint8))

        def run(leg):
            if leg == "a":
                plan.execute_power(d_in, nbytes, width, d_plane)
            elif leg == "b":
                plan.execute_occupancy(d_in, nbytes, width, d_thr, full, d_rows, d_frames)
            elif leg == "c_rows":
                ctx.power_occupancy(d_plane, n, width, d_thr, [], d_rows + 4 * n, 0)
            elif leg == "c_frames":
                ctx.power_occupancy(d_plane, n, width, d_thr, full, 0, d_frames + 4 * width)
            elif leg == "c_both":
                ctx.power_occupancy(d_plane, n, width, d_thr, full, d_rows + 2 * 4 * n, d_frames + 2 * 4 * width)
            elif leg == "c_both8":
                ctx.power_occupancy(d_plane, n, width, d_thr, eighths, d_rows + 3 * 4 * n, d_frames + 3 * 4 * width)
            elif leg == "t":
                ctx.power_tracks(d_plane, n, width, full, d_row, d_peak)
            else:
                ctx.power_mean(d_plane, n, width, d_mean)
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
        rows = ctx.download(d_rows, 4 * 4 * n, np.uint32).reshape(4, n)
        frames = ctx.download(d_frames, 11 * 4 * width, np.uint32).reshape(11, width)
        plane_bytes = 8 * width * n
        hits = int(rows[0].astype(np.int64).sum())
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width,
               "kernel_a": plan.power_kernel_name_for(nbytes, width), "kernel_b": plan.occupancy_kernel_name_for(nbytes, width),
               "a_power_ms": round(best["a"], 4), "b_occupancy_ms": round(best["b"], 4), "c_rows_ms": round(best["c_rows"], 4),
               "c_frames_ms": round(best["c_frames"], 4), "c_both_ms": round(best["c_both"], 4), "c_both8_ms": round(best["c_both8"], 4),
               "t_power_tracks_ms": round(best["t"], 4), "m_power_mean_ms": round(best["m"], 4),
               "b_over_a": round(best["b"] / best["a"], 4), "c_both_over_t": round(best["c_both"] / best["t"], 4),
               "c_both_over_m": round(best["c_both"] / best["m"], 4), "c_both8_over_c_both": round(best["c_both8"] / best["c_both"], 4),
               "plane_bytes": plane_bytes, "c_both_plane_gb_s": round(plane_bytes / (best["c_both"] * 1e-3) / 1e9, 1),
               "t_plane_gb_s": round(plane_bytes / (best["t"] * 1e-3) / 1e9, 1),
               "b_equals_c": bool((rows[0] == rows[2]).all() and (rows[0] == rows[1]).all() and (rows[0] == rows[3]).all()
                                  and (frames[0] == frames[2]).all() and (frames[0] == frames[1]).all()
                                  and (frames[3:11].astype(np.int64).sum(axis=0) == frames[0]).all()),
               "hit_share": round(hits / float(width * n), 4), "frames_hold_the_rows": bool(int(frames[0].astype(np.int64).sum()) == hits),
               "reps": args.reps}
        if os.environ.get("SP_LIB_VARIANT") and os.environ.get("SP_EXPERIMENT_KNOBS") == "1":
            rec["variant"] = os.environ["SP_LIB_VARIANT"]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_plane, d_rows, d_frames, d_mean, d_thr, d_row, d_peak, d_in):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
