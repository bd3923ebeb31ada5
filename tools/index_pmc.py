#!/usr/bin/env python3
"""One leg of tools/index_bench.py over and over, for a counters-only profiler run (rocprofv3 --pmc WRITE_SIZE FETCH_SIZE -- python3
tools/index_pmc.py LEG SHAPE): the HBM traffic of the RGBA write-out (leg a, sp_plan_execute) against the index write-out (leg b,
sp_plan_execute_index) on the same capture.  Prints the bytes each image holds, to set the counters against.
SHAPE: cfg2 | cfg2_wf | cfg4 | cfg4_wf | cfg3 | cfg3_wf   (a 2^26-sample config-4 slice)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SHAPES = {"cfg2": ("CF32", 24, 1024, "blackmanHarris"), "cfg4": ("CU8", 26, 1024, "blackmanHarris"), "cfg3": ("CS16", 26, 2048, "hann")}


def main():
    leg, shape = sys.argv[1], sys.argv[2]
    wf = shape.endswith("_wf")
    fmt, log2s, n, window = SHAPES[shape.replace("_wf", "")]
    pkg = load_package()
    ctx = pkg.Context(0)
    sw = pkg.parse_format(fmt)[1]
    samples = 1 << log2s
    width = samples // n
    d_in = ctx.alloc(samples * sw)
    ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
    win, weight = pkg.window(window, n)
    lut = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 3) & 255], axis=1).astype(np.uint8)
    d_img = ctx.alloc(4 * width * n)
    small = {k: ctx.alloc(max(v, 16)) for k, v in (("gauge_mins", width), ("gauge_maxs", width), ("gauge_amps", width),
                                                    ("c_hist", 8 * 256), ("cb_hist", 8000), ("dbfs_minmax", 16))}
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut, False, wf)
    for _ in range(5):
        if leg == "a":
            plan.execute(d_in, samples * sw, width, rgba=d_img, **small)
        else:
            plan.execute_index(d_in, samples * sw, width, index=d_img, **small)
        ctx.synchronize()
    print("leg %s shape %s: capture %d bytes, image %d bytes" % (leg, shape, samples * sw, (4 if leg == "a" else 1) * width * n))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
