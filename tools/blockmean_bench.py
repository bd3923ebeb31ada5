#!/usr/bin/env python3
"""The averaged spectrogram against the replies at its two ends: JSON lines per shape and group (profiles/blockmean_bench.jsonl).

Legs, device-resident, in one process behind one spin-up, HIP events around each call's launches, best of 5 after a warm-up, interleaved:
  a   sp_plan_execute_power into a resident plane - the yardstick, unchanged code
  b   sp_plan_execute_blockmean on the same request (the plane passes through the window)
  c   sp_power_blockmean on a's plane
  d   sp_power_mean on a's plane - the yardstick of the carried path: c at group = width is the same launches
  e   torch's plane.view(columns, group, n).mean(1), where group divides the width - NOT exact, for scale only; torch's own events
  f   sp_plan_power_to_index on a's plane, beside sp_plan_execute_index of the same request (f_index)
b and c run at direct_max = 1 (every column carried) and 2^30 (every whole column through k_blockmean); the crossover between the two is
where SP_BLOCKMEAN_DIRECT_FRAMES is set.  c, d, e and f read a plane the leg before has just written or read: the planes here are 16 MiB
and 128 MiB, below the part's 256 MiB of last-level cache, so these are cache-resident figures and say nothing certain about HBM.
Shapes: tools/occupancy_bench.py's three; groups 2, 8, 64, 256, 512, 1024 and the width.
Usage: tools/blockmean_bench.py [--out FILE] [--reps 5] [--shape NAME]
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
DIRECT = (("carried", 1), ("direct", 1 << 30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="")
    args = ap.parse_args()
    try:                                  # (leg e: torch opens the device first, where there is a torch)
        import torch
        have_torch = torch.cuda.is_available()
    except ImportError:
        torch, have_torch = None, False
    pkg = load_package()
    ctx = pkg.Context(0)
    ctx.enable_timing(True)
    lut = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)
    lines = []
    spun = False
    for name, fmt, log2s, n, window, width in SHAPES:
        if args.shape and name != args.shape:
            continue
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        plane_bytes = 8 * width * n
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        d_plane, d_out, d_mean, d_ix = ctx.alloc(plane_bytes), ctx.alloc(plane_bytes), ctx.alloc(8 * n), ctx.alloc(width * n)
        small = {k: ctx.alloc(max(v, 16)) for k, v in (("gauge_mins", width), ("gauge_maxs", width), ("gauge_amps", width),
                                                        ("c_hist", 8 * 256), ("cb_hist", 8000), ("dbfs_minmax", 16))}
        plan.execute_power(d_in, nbytes, width, d_plane)
        ctx.synchronize()
        t_plane = None
        if have_torch:
            t_plane = torch.from_numpy(ctx.download(d_plane, plane_bytes, np.float64).reshape(width, n).copy()).to("cuda")
            ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed_call(call):
            call()
            ctx.synchronize()
            return ctx.last_kernel_ms()

        def torch_mean(group):
            ev[0].record()
            t_plane.view(width // group, group, n).mean(1)
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])

        def best_of(legs):
            """{leg: best ms} of the callables in `legs`, warmed up once each and then interleaved."""
            for call in legs.values():
                call()
            best = {}
            for _ in range(args.reps):
                for leg, call in legs.items():
                    best[leg] = min(best.get(leg, 1e30), call())
            return best

        t_end = time.time() + (0.0 if spun else 0.5)   # one spin-up: the clocks ramp over the first few hundred milliseconds
        while time.time() < t_end:
            timed_call(lambda: plan.execute_power(d_in, nbytes, width, d_plane))
        spun = True
        base = best_of({"a": lambda: timed_call(lambda: plan.execute_power(d_in, nbytes, width, d_plane)),
                        "d": lambda: timed_call(lambda: ctx.power_mean(d_plane, n, width, d_mean)),
                        "f": lambda: timed_call(lambda: plan.power_to_index(d_plane, width, d_ix)),
                        "f_index": lambda: timed_call(lambda: plan.execute_index(d_in, nbytes, width, index=d_ix, **small))})
        gbs = lambda ms: round(plane_bytes / ms / 1e6, 1)  # noqa: E731
        rec = {"shape": name, "format": fmt, "n": n, "samples": samples, "width": width, "plane_bytes": plane_bytes, "reps": args.reps,
               "a_power_ms": round(base["a"], 4), "d_power_mean_ms": round(base["d"], 4), "d_plane_GBps": gbs(base["d"]),
               "f_power_to_index_ms": round(base["f"], 4), "f_plane_GBps": gbs(base["f"]), "f_execute_index_ms": round(base["f_index"], 4),
               "kernel_b": plan.blockmean_kernel_name_for(nbytes, width)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        for group in (2, 8, 64, 256, 512, 1024, width):
            rec = {"shape": name, "group": group, "columns": pkg.binding.blockmean_columns(width, group)}
            bits = {}
            for label, direct_max in DIRECT:
                ctx.set_blockmean_direct_max(direct_max)
                legs = {"a": lambda: timed_call(lambda: plan.execute_power(d_in, nbytes, width, d_plane)),
                        "b": lambda: timed_call(lambda: plan.execute_blockmean(d_in, nbytes, width, group, d_out)),
                        "c": lambda: timed_call(lambda: ctx.power_blockmean(d_plane, n, width, group, d_out)),
                        "d": lambda: timed_call(lambda: ctx.power_mean(d_plane, n, width, d_mean))}
                if have_torch and label == "direct":
                    legs["e"] = lambda: torch_mean(group)
                best = best_of(legs)
                bits[label] = ctx.download(d_out, 8 * rec["columns"] * n, np.uint64)
                rec.update({"a_ms_" + label: round(best["a"], 4), "b_ms_" + label: round(best["b"], 4), "c_ms_" + label: round(best["c"], 4),
                            "c_plane_GBps_" + label: gbs(best["c"]), "d_ms_" + label: round(best["d"], 4),
                            "d_plane_GBps_" + label: gbs(best["d"])})
                if "e" in best:
                    rec["e_torch_mean_ms"] = round(best["e"], 4)
            ctx.set_blockmean_direct_max(0)
            rec["same_bits"] = bool((bits["carried"] == bits["direct"]).all())
            rec["direct_over_carried_c"] = round(rec["c_ms_direct"] / rec["c_ms_carried"], 4)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        plan.close()
        for p in [d_in, d_plane, d_out, d_mean, d_ix] + list(small.values()):
            ctx.free(p)
        t_plane = None
    ctx.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
