#!/usr/bin/env python3
"""The burst measurements against the burst lists they run behind: one JSON line per shape (profiles/pulse_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  a   sp_plan_execute_bursts - the yardstick: the code leg b runs in front of its own launches, unchanged
  b   sp_plan_execute_pulses on the same request (a's launches, then a memset, k_pulse_accumulate, k_pulse_peak_frame, k_pulse_finish)
  c   sp_series_bursts alone on the request's band series
  d   sp_series_pulses on the same series
and two alternatives on the same device, for scale:
  e   copying the band series to the host (what a caller did for a burst's level before), wall clock around the copy
  f   torch.segment_reduce "sum" and "max" over the band of most bursts, its lengths made on the host from that band's edges - where
      this torch build has it; HIP events of torch's around the two calls (not counted: making the lengths)
The series has just been written or read by the leg before: where it fits the caches the figures are cache-resident ones and say nothing
about HBM.  Thresholds: every band series' own median times 2 (hi) and times 1 (lo); the shapes named *_long have hi = lo = 0 instead, ONE
burst per band over every frame - the contention case.  b and d must give the same words, and a's words.
Shapes: tools/burst_bench.py's five and the long burst at width 2^20 with one band and with 64.
Usage: tools/pulse_bench.py [--out FILE] [--reps 5] [--shape NAME]
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

# (name, format, log2 of the samples, n, window, width, bands, max_bursts, one long burst per band)
SHAPES = (("cf32_w16384", "CF32", 24, 1024, "blackmanHarris", 16384, 8, 4096, False),
          ("cf32_w2048", "CF32", 24, 1024, "blackmanHarris", 2048, 8, 4096, False),
          ("cu8_w4096", "CU8", 24, 512, "hann", 4096, 8, 4096, False),
          ("cu8_w1m_1band", "CU8", 24, 64, "hann", 1 << 20, 1, 4096, False),
          ("cu8_w1m_1band_long", "CU8", 24, 64, "hann", 1 << 20, 1, 4096, True),
          ("cu8_w1m_64bands", "CU8", 24, 64, "hann", 1 << 20, 64, 1 << 17, False),
          ("cu8_w1m_64bands_long", "CU8", 24, 64, "hann", 1 << 20, 64, 16, True))
LEGS = ("a", "b", "c", "d", "e", "f")


def bands_of(n, count):
    if count == 8:
        return [(0, n), (0, 1), (1, 64), (3, 68), (n - 1, n), (0, n // 2 + 1), (n // 4, n), (n // 2, n // 2 + 8)]
    if count == 1:
        return [(n // 4, n // 2)]
    return [(k * n // count, (k + 1) * n // count) for k in range(count)]


def segment_reduce_leg(series_row, edges_row, total, width):
    """(a function that runs the two reductions and returns their milliseconds, "") or (None, why not)."""
    try:
        import torch
    except ImportError as e:
        return None, "no torch: %s" % e
    if not hasattr(torch, "segment_reduce") or not torch.cuda.is_available():
        return None, "this torch build has no segment_reduce" if torch.cuda.is_available() else "torch sees no device"
    e = edges_row[:min(int(total), len(edges_row))].astype(np.int64).reshape(-1)
    cuts = np.concatenate(([0], e, [width]))                  # gap, burst, gap, ... : every frame lies in one segment
    lengths = torch.from_numpy(np.diff(cuts)).to("cuda")
    data = torch.from_numpy(np.array(series_row)).to("cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        start.record()
        torch.segment_reduce(data, "sum", lengths=lengths, unsafe=True)
        torch.segment_reduce(data, "max", lengths=lengths, unsafe=True)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)
    try:
        run()
    except Exception as e:   # noqa: BLE001 (whatever this build refuses: the leg is an aside)
        return None, "torch.segment_reduce failed: %s" % str(e)[:200]
    return run, ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="")
    args = ap.parse_args()
    try:                                  # (leg f: torch opens the device first, where there is a torch)
        import torch
        torch.cuda.is_available()
    except ImportError:
        pass
    pkg = load_package()
    ctx = pkg.Context(0)
    ctx.enable_timing(True)
    lut = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)
    lines = []
    spun = False
    for name, fmt, log2s, n, window, width, count, m, long_burst in SHAPES:
        if args.shape and name != args.shape:
            continue
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        bands = bands_of(n, count)
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        d_series = ctx.alloc(8 * count * width)
        per = count * m
        # two sets of outputs: [0] the plan's legs a and b, [1] the series' legs c and d
        d_counts, d_edges = ctx.alloc(4 * count * 2), ctx.alloc(8 * per * 2)
        d_energy, d_peak, d_at = ctx.alloc(8 * per * 2), ctx.alloc(8 * per * 2), ctx.alloc(4 * per * 2)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        plan.execute_bandpower(d_in, nbytes, width, bands, d_series)
        ctx.synchronize()
        series = ctx.download(d_series, 8 * count * width, np.float64).reshape(count, width)
        lo = np.zeros(count) if long_burst else np.sort(series, axis=1)[:, (width - 1) // 2].copy()
        hi = 2.0 * lo
        outs = lambda k: (d_counts + 4 * count * k, d_edges + 8 * per * k, d_energy + 8 * per * k, d_peak + 8 * per * k,  # noqa: E731
                          d_at + 4 * per * k)
        plan.execute_bursts(d_in, nbytes, width, bands, hi, lo, m, *outs(0)[:2])
        ctx.synchronize()
        totals = ctx.download(d_counts, 4 * count, np.uint32)
        busiest = int(np.argmax(totals))
        edges_busiest = ctx.download(d_edges, 8 * per, np.int32).reshape(count, m, 2)[busiest]
        reduce_leg, reduce_note = segment_reduce_leg(series[busiest], edges_busiest, totals[busiest], width)

        def run(leg):
            if leg == "a":
                plan.execute_bursts(d_in, nbytes, width, bands, hi, lo, m, *outs(0)[:2])
            elif leg == "b":
                plan.execute_pulses(d_in, nbytes, width, bands, hi, lo, m, *outs(0))
            elif leg == "c":
                ctx.series_bursts(d_series, count, width, hi, lo, m, *outs(1)[:2])
            elif leg == "d":
                ctx.series_pulses(d_series, count, width, hi, lo, m, *outs(1))
            elif leg == "e":
                t0 = time.perf_counter()
                ctx.download(d_series, 8 * count * width, np.float64)
                return (time.perf_counter() - t0) * 1e3
            else:
                return reduce_leg() if reduce_leg else float("nan")
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
        got = [[ctx.download(p + size * k, size, t) for k in (0, 1)]
               for p, size, t in ((d_counts, 4 * count, np.uint32), (d_edges, 8 * per, np.int32), (d_energy, 8 * per, np.uint64),
                                  (d_peak, 8 * per, np.uint64), (d_at, 4 * per, np.int32))]
        listed = np.minimum(got[0][0], m)
        r = lambda v: None if v != v else round(v, 4)  # noqa: E731
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width, "bands": count, "max_bursts": m,
               "long_burst": long_burst, "segment_frames": pkg.binding.SP_BURST_SEGMENT_FRAMES, "zeroing": "hipMemsetAsync of the whole workspace",
               "kernel_b": plan.pulses_kernel_name_for(nbytes, width),
               "a_bursts_ms": r(best["a"]), "b_pulses_ms": r(best["b"]), "c_series_bursts_ms": r(best["c"]), "d_series_pulses_ms": r(best["d"]),
               "e_copy_series_to_host_ms": r(best["e"]), "f_torch_segment_reduce_one_band_ms": r(best["f"]) if reduce_leg else None, "f_note": reduce_note,
               "b_over_a": r(best["b"] / best["a"]), "d_over_c": r(best["d"] / best["c"]), "b_minus_a_ms": r(best["b"] - best["a"]),
               "d_minus_c_ms": r(best["d"] - best["c"]), "series_bytes": 8 * count * width, "workspace_bytes": 8 * 69 * per + 4 * count,
               "bursts_total": int(got[0][0].sum()), "bursts_most": int(got[0][0].max()), "bursts_listed": int(listed.sum()),
               "b_equals_d": bool(all((g[0] == g[1]).all() for g in got)), "reps": args.reps}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        plan.close()
        for p in (d_in, d_series, d_counts, d_edges, d_energy, d_peak, d_at):
            ctx.free(p)
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
