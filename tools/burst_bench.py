#!/usr/bin/env python3
"""The burst lists against the power plane and the band-power series they are made of: one JSON line per shape
(profiles/burst_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  a   sp_plan_execute_power into a resident plane (one launch, 8 bytes per bin)
  b   sp_plan_execute_bandpower with the default window - the yardstick: the code leg c runs in front of its three launches
  c   sp_plan_execute_bursts (b's launches into the workspace series, then k_burst_summary, k_burst_carry, k_burst_emit)
  d   sp_series_bursts alone on b's series: the three launches, 8 * count * width bytes read twice
  e   sp_power_bands on a's plane: one launch, 8 * n * width bytes read once
The series and the plane have just been written or read by the leg before: where they fit the caches the figures are cache-resident
ones and say nothing about HBM.  Thresholds: every band series' own median times 2 (hi) and times 1 (lo).  c and d must give the same
words.
Shapes: tools/occupancy_bench.py's three with eight bands, and a width of 2^20 frames (n = 64, one frame every 16 samples) with one band
and with 64 bands of one row.
A library built with another segment size (tools/build_variant.sh NAME "-DSP_BURST_SEGMENT_FRAMES=1024", loaded with
SP_EXPERIMENT_KNOBS=1 SP_LIB_VARIANT=NAME) is measured by the same command; --segment N labels its lines.
Usage: tools/burst_bench.py [--out FILE] [--reps 5] [--shape NAME] [--segment N]
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

# (name, format, log2 of the samples, n, window, width, bands: 8 standard ones or that many of one row)
SHAPES = (("cf32_w16384", "CF32", 24, 1024, "blackmanHarris", 16384, 8), ("cf32_w2048", "CF32", 24, 1024, "blackmanHarris", 2048, 8),
          ("cu8_w4096", "CU8", 24, 512, "hann", 4096, 8), ("cu8_w1m_1band", "CU8", 24, 64, "hann", 1 << 20, 1),
          ("cu8_w1m_64bands", "CU8", 24, 64, "hann", 1 << 20, 64))
LEGS = ("a", "b", "c", "d", "e")
MAX_BURSTS = 4096


def bands_of(n, count):
    if count == 8:
        return [(0, n), (0, 1), (1, 64), (3, 68), (n - 1, n), (0, n // 2 + 1), (n // 4, n), (n // 2, n // 2 + 8)]
    if count == 1:
        return [(n // 4, n // 2)]
    return [(k * n // count, (k + 1) * n // count) for k in range(count)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="")
    ap.add_argument("--segment", type=int, default=0)
    args = ap.parse_args()
    pkg = load_package()
    ctx = pkg.Context(0)
    ctx.enable_timing(True)
    lut = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)
    lines = []
    spun = False
    for name, fmt, log2s, n, window, width, count in SHAPES:
        if args.shape and name != args.shape:
            continue
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        bands = bands_of(n, count)
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        d_plane, d_series, d_series_e = ctx.alloc(8 * width * n), ctx.alloc(8 * count * width), ctx.alloc(8 * count * width)
        d_counts, d_edges = ctx.alloc(4 * count * 2), ctx.alloc(8 * count * MAX_BURSTS * 2)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        plan.execute_bandpower(d_in, nbytes, width, bands, d_series)
        ctx.synchronize()
        series = ctx.download(d_series, 8 * count * width, np.float64).reshape(count, width)
        lo = np.sort(series, axis=1)[:, (width - 1) // 2].copy()
        hi = 2.0 * lo

        def run(leg):
            if leg == "a":
                plan.execute_power(d_in, nbytes, width, d_plane)
            elif leg == "b":
                plan.execute_bandpower(d_in, nbytes, width, bands, d_series)
            elif leg == "c":
                plan.execute_bursts(d_in, nbytes, width, bands, hi, lo, MAX_BURSTS, d_counts, d_edges)
            elif leg == "d":
                ctx.series_bursts(d_series, count, width, hi, lo, MAX_BURSTS, d_counts + 4 * count, d_edges + 8 * count * MAX_BURSTS)
            else:
                ctx.power_bands(d_plane, n, width, bands, d_series_e)
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
        counts = ctx.download(d_counts, 4 * count * 2, np.uint32).reshape(2, count)
        edges = ctx.download(d_edges, 8 * count * MAX_BURSTS * 2, np.int32).reshape(2, -1)
        r = lambda v: round(v, 4)  # noqa: E731
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width, "bands": count, "max_bursts": MAX_BURSTS,
               "segment_frames": args.segment or pkg.binding.SP_BURST_SEGMENT_FRAMES, "carry": "own launch (k_burst_carry)",
               "kernel_c": plan.bursts_kernel_name_for(nbytes, width),
               "a_power_ms": r(best["a"]), "b_bandpower_ms": r(best["b"]), "c_bursts_ms": r(best["c"]), "d_series_bursts_ms": r(best["d"]),
               "e_power_bands_ms": r(best["e"]), "c_over_b": r(best["c"] / best["b"]), "d_over_e": r(best["d"] / best["e"]),
               "c_minus_b_ms": r(best["c"] - best["b"]), "series_bytes": 8 * count * width, "plane_bytes": 8 * n * width,
               "d_series_gb_s_two_reads": round(2 * 8 * count * width / (best["d"] * 1e-3) / 1e9, 1),
               "bursts_total": int(counts[0].sum()), "bursts_most": int(counts[0].max()),
               "c_equals_d": bool((counts[0] == counts[1]).all() and (edges[0] == edges[1]).all()), "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_in, d_plane, d_series, d_series_e, d_counts, d_edges):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "a" if args.segment else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
