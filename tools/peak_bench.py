#!/usr/bin/env python3
"""Peak detector against the only other route to the same picture: one JSON line per shape (profiles/peak_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around the kernel, best of 5 after a warm-up:
  a  sp_plan_execute, detector = sample, width * M columns of the capture (as many transforms, M times the pixels and epilogues)
  b  sp_plan_execute, detector = peak, width columns
  c  sp_plan_execute, detector = sample, width columns (what the hold costs over the reference's sparse picture)
n = 512 is also measured at 4 096 columns: launch_frames' rule makes 16-column groups there, so 2 048 columns are 128 workgroups on 256
CUs and 4 096 columns are 256 (the record's "groups" is that count).
Usage: tools/peak_bench.py [--out FILE] [--reps 5]
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
    for fmt in ("CU8", "CF32"):
        sw = pkg.parse_format(fmt)[1]
        for log2s in (24, 28):
            samples = 1 << log2s
            nbytes = samples * sw
            d_in = ctx.alloc(nbytes)
            ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
            for n, width in ((512, 2048), (1024, 2048), (512, 4096)):
                win, weight = pkg.window("blackmanHarris", n)
                M, last = pkg.binding.peak_subframes(fmt, n, nbytes, width)
                wide = width * M
                d_img = ctx.alloc(4 * wide * n)
                small = {k: ctx.alloc(max(v, 16)) for k, v in (("gauge_mins", wide), ("gauge_maxs", wide), ("gauge_amps", wide),
                                                                ("c_hist", 8 * 256), ("cb_hist", 8000), ("dbfs_minmax", 16))}
                plans = {"sample": ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 60.0, lut),
                         "peak": ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 60.0, lut, detector="peak")}
                legs = {"a": ("sample", wide), "b": ("peak", width), "c": ("sample", width)}

                def run(leg):
                    det, w = legs[leg]
                    plans[det].execute(d_in, nbytes, w, rgba=d_img, **small)
                    ctx.synchronize()
                    return ctx.last_kernel_ms()

                t_end = time.time() + 0.5                      # spin-up: the clocks ramp over the first few hundred milliseconds
                while time.time() < t_end:
                    run("c")
                best = {}
                for leg in legs:
                    run(leg)                                   # warm-up of this leg
                for _ in range(args.reps):                     # the legs interleaved: a drift of the box hits all three alike
                    for leg in legs:
                        ms = run(leg)
                        best[leg] = min(best.get(leg, 1e30), ms)
                rec = {"format": fmt, "n": n, "samples": samples, "width": width, "M": M, "last_column_count": last,
                       "groups": -(-width // (16 if n == 512 else 8)),       # workgroups of leg b (frames per round of 512 threads)
                       "kernel_a": plans["sample"].kernel_name(nbytes, wide), "kernel_b": plans["peak"].kernel_name(nbytes, width),
                       "a_wide_sample_ms": round(best["a"], 4), "b_peak_ms": round(best["b"], 4), "c_sample_ms": round(best["c"], 4),
                       "b_over_a": round(best["b"] / best["a"], 4), "reps": args.reps}
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
                for p in plans.values():
                    p.close()
                for p in list(small.values()) + [d_img]:
                    ctx.free(p)
            ctx.free(d_in)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
