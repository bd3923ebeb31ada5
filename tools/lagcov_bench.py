#!/usr/bin/env python3
"""The exact lagged covariances against the exact variance sums in the same run: one JSON line per series size, then one per plan shape
(profiles/lagcov_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  pv      sp_power_variance on a resident plane of 16 384 frames of n = 1024 (a memset, k_variance_accumulate, k_variance_finish) - the
          yardstick: both accumulations do eight LDS atomics per item, so its VALUES per second stand beside the TERMS per second of
  s_small sp_series_lagcov, 1 pair of 64 lags, on the 16 384-frame series of the same plane's bands (a memset, k_lagcov_accumulate,
          k_lagcov_finish)
  s_large sp_series_lagcov, 16 pairs of 1024 lags, on the same series
The two sizes give a fixed part and a rate: time = fixed + terms / rate, solved from the two lines, derived and not measured per kernel.
Then, on tools/band_bench.py's shapes:
  eb      sp_plan_execute_bandpower with the default window - the yardstick of el
  el      sp_plan_execute_lagcov, 4 pairs of 64 lags (the same frame loop and band sums block by block, the two launches behind)
Usage: tools/lagcov_bench.py [--out FILE] [--reps 5]
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
SIZES = (("s_small", 1, 64), ("s_large", 16, 1024))


def _bands(n, count):
    step = n // count
    return [(k * step, (k + 1) * step) for k in range(count)]


def _pairs(npairs, count):
    return [(k % count, (k * 3 + k // count) % count) for k in range(npairs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = load_package()
    b = pkg.binding
    ctx = pkg.Context(0)
    ctx.enable_timing(True)
    lut = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)
    lines = []

    # ---- the series legs against the variance of the plane the series comes from
    name, fmt, log2s, n, window, width = SHAPES[0]
    sw = pkg.parse_format(fmt)[1]
    samples = 1 << log2s
    nbytes = samples * sw
    count = 8
    bands = _bands(n, count)
    d_in = ctx.alloc(nbytes)
    ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
    win, weight = pkg.window(window, n)
    d_plane, d_var, d_series = ctx.alloc(8 * width * n), ctx.alloc(3 * 8 * n), ctx.alloc(8 * count * width)
    d_out = ctx.alloc(3 * 8 * b.SP_MAX_LAG_PAIRS * b.SP_MAX_LAGS)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
    plan.execute_power(d_in, nbytes, width, d_plane)
    ctx.power_bands(d_plane, n, width, bands, d_series)
    ctx.synchronize()

    def run(leg):
        if leg == "pv":
            ctx.power_variance(d_plane, n, width, d_var)
        else:
            _, npairs, lags = next(s for s in SIZES if s[0] == leg)
            ctx.series_lagcov(d_series, count, width, _pairs(npairs, count), lags, d_out)
        ctx.synchronize()
        return ctx.last_kernel_ms()

    t_end = time.time() + 0.5                          # one spin-up: the clocks ramp over the first few hundred milliseconds
    while time.time() < t_end:
        run("pv")
    legs = ("pv",) + tuple(s[0] for s in SIZES)
    best = {}
    for leg in legs:
        run(leg)                                       # warm-up of this leg
    for _ in range(args.reps):                         # the legs interleaved: a drift of the box hits all alike
        for leg in legs:
            best[leg] = min(best.get(leg, 1e30), run(leg))
    values = width * n
    terms = {}
    for leg, npairs, lags in SIZES:
        terms[leg] = npairs * lags * b.lagcov_terms(width, lags)
        rec = {"shape": leg, "series_frames": width, "bands": count, "npairs": npairs, "lags": lags, "terms_per_lag": b.lagcov_terms(width, lags),
               "terms": terms[leg], "launch": list(b.debug_lagcov_launch(npairs, lags, b.lagcov_terms(width, lags), 256)), "reps": args.reps,
               "ms": round(best[leg], 4), "terms_per_s": round(terms[leg] / (best[leg] * 1e-3), 0),
               "pv_ms": round(best["pv"], 4), "pv_values": values, "pv_values_per_s": round(values / (best["pv"] * 1e-3), 0)}
        rec["terms_rate_over_pv_values_rate"] = round(rec["terms_per_s"] / rec["pv_values_per_s"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    (s0, _, _), (s1, _, _) = SIZES
    rate = (terms[s1] - terms[s0]) / ((best[s1] - best[s0]) * 1e-3)
    rec = {"shape": "derived", "what": "time = fixed + terms / rate from the two sizes", "rate_terms_per_s": round(rate, 0),
           "fixed_ms": round(best[s0] - terms[s0] / rate * 1e3, 4)}
    print(json.dumps(rec), flush=True)
    lines.append(json.dumps(rec))
    plan.close()
    for p in (d_plane, d_var, d_series, d_out, d_in):
        ctx.free(p)

    # ---- through the plan, against the band-power series
    for name, fmt, log2s, n, window, width in SHAPES:
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        count, npairs, lags = 8, 4, 64
        bands, pairs = _bands(n, count), _pairs(4, 8)
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        d_band, d_out = ctx.alloc(8 * count * width), ctx.alloc(3 * 8 * npairs * lags)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)

        def run_plan(leg):
            if leg == "eb":
                plan.execute_bandpower(d_in, nbytes, width, bands, d_band)
            else:
                plan.execute_lagcov(d_in, nbytes, width, bands, pairs, lags, d_out)
            ctx.synchronize()
            return ctx.last_kernel_ms()

        best = {}
        for leg in ("eb", "el"):
            run_plan(leg)
        for _ in range(args.reps):
            for leg in ("eb", "el"):
                best[leg] = min(best.get(leg, 1e30), run_plan(leg))
        # the reply is the one sp_series_lagcov gives on the band-power series of the last eb leg, bit for bit
        d_check = ctx.alloc(3 * 8 * npairs * lags)
        ctx.series_lagcov(d_band, count, width, pairs, lags, d_check)
        ctx.synchronize()
        same = bool((ctx.download(d_check, 3 * 8 * npairs * lags, np.uint64) == ctx.download(d_out, 3 * 8 * npairs * lags, np.uint64)).all())
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width, "bands": count, "npairs": npairs, "lags": lags,
               "kernel_el": plan.lagcov_kernel_name_for(nbytes, width), "reps": args.reps, "eb_ms": round(best["eb"], 4),
               "el_ms": round(best["el"], 4), "el_over_eb": round(best["el"] / best["eb"], 3), "equals_series_lagcov_of_bandpower": same}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_band, d_out, d_check, d_in):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
