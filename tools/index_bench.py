#!/usr/bin/env python3
"""Indexed image replies against the RGBA render of the same request: one JSON line per shape (profiles/index_bench.jsonl).

Device legs, device-resident, in one process behind one spin-up, HIP events around the launches, best of --reps after a warm-up,
interleaved:
  a   sp_plan_execute (k_frames: the RGBA write-out)          a2  the same leg again: |a2 / a - 1| is the run's noise margin
  b   sp_plan_execute_index (k_frames_index)                  f   the same request forced onto render_extract
Shapes: BASELINE config 1 (cu8, 2^20 samples, n = 512), config 2 (cf32, 2^24 samples, n = 1024), config 2's capture at 2 048 columns,
one config-4 slice (cu8, 2^28 samples, n = 1024, width 262 144) and config 3 (cs16, n = 2048, a 2^26-sample slice), each in both layouts.
Host legs (--host), by the host clock after a warm-up, with pageable and with page-locked buffers (capture and every reply buffer):
c sp_render, d sp_render_index, for cu8 n = 1024 at 2^26 samples and for config 2.
Usage: tools/index_bench.py [--out FILE] [--reps 5] [--host]
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

SHAPES = (("cfg1", "CU8", 20, 512, "hann", None), ("cfg2", "CF32", 24, 1024, "blackmanHarris", None),
          ("cfg2_w2048", "CF32", 24, 1024, "blackmanHarris", 2048), ("cfg4_slice", "CU8", 28, 1024, "blackmanHarris", None),
          ("cfg3_slice", "CS16", 26, 2048, "hann", None))
HOST_SHAPES = (("cu8_n1024_2^26", "CU8", 26, 1024, "blackmanHarris"), ("cfg2", "CF32", 24, 1024, "blackmanHarris"))


def device_legs(pkg, ctx, lut, reps, emit):
    spun = False
    for name, fmt, log2s, n, window, width in SHAPES:
        sw = pkg.parse_format(fmt)[1]
        samples = 1 << log2s
        nbytes = samples * sw
        width = width or samples // n
        d_in = ctx.alloc(nbytes)
        ctx.synth_trinoise(d_in, fmt, 0, samples, 4242, 7321, 11, 0.5, 0.02)
        win, weight = pkg.window(window, n)
        d_img = ctx.alloc(4 * width * n)
        d_ix = ctx.alloc(width * n)
        small = {k: ctx.alloc(max(v, 16)) for k, v in (("gauge_mins", width), ("gauge_maxs", width), ("gauge_amps", width),
                                                        ("c_hist", 8 * 256), ("cb_hist", 8000), ("dbfs_minmax", 16))}
        for wf in (False, True):
            plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut, False, wf)
            forced = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut, False, wf)
            forced.force_kernel("scratch")

            def run(leg):
                if leg in ("a", "a2"):
                    plan.execute(d_in, nbytes, width, rgba=d_img, **small)
                elif leg == "b":
                    plan.execute_index(d_in, nbytes, width, index=d_ix, **small)
                else:
                    forced.execute_index(d_in, nbytes, width, index=d_ix, **small)
                ctx.synchronize()
                return ctx.last_kernel_ms()

            t_end = time.time() + (0.0 if spun else 0.5)   # one spin-up: the clocks ramp over the first few hundred milliseconds
            while time.time() < t_end:
                run("a")
            spun = True
            legs = ("a", "b", "f", "a2")
            best = {}
            for leg in legs:
                run(leg)                                   # warm-up of this leg (workspaces, the identity LUT)
            for _ in range(reps):                          # the legs interleaved: a drift of the box hits all alike
                for leg in legs:
                    best[leg] = min(best.get(leg, 1e30), run(leg))
            emit({"shape": name + ("_wf" if wf else ""), "format": fmt, "n": n, "samples": samples, "width": width, "waterfall": wf,
                  "kernel_b": plan.index_kernel_name_for(nbytes, width), "kernel_f": forced.index_kernel_name_for(nbytes, width),
                  "a_rgba_ms": round(best["a"], 4), "b_index_ms": round(best["b"], 4), "f_extract_ms": round(best["f"], 4),
                  "b_over_a": round(best["b"] / best["a"], 4), "b_over_f": round(best["b"] / best["f"], 4),
                  "noise_a2_over_a": round(best["a2"] / best["a"], 4), "reps": reps})
            plan.close()
            forced.close()
        for p in list(small.values()) + [d_img, d_ix, d_in]:
            ctx.free(p)


def host_legs(pkg, ctx, lut, reps, emit):
    """c / d through the C ABI itself, so that the capture and every reply buffer can lie in page-locked memory (sp_host_alloc)."""
    import ctypes as C
    b = pkg.binding
    L = ctx.lib.L
    rng = np.random.default_rng(7)
    for name, fmt, log2s, n, window in HOST_SHAPES:
        fid, sw = pkg.parse_format(fmt)
        samples = 1 << log2s
        width = samples // n
        src = rng.integers(0, 256, samples * sw, dtype=np.uint8)
        if fmt == "CF32":
            src = (rng.standard_normal(2 * samples).astype(np.float32) * 0.3).view(np.uint8)
        win, weight = pkg.window(window, n)
        req, keep = b._make_request(fid, n, win, 1.0 / weight, 6.0, 30.0, lut, False, False)
        sizes = [src.size, 4 * width * n, width * n, width, width, width, 8 * 256, 8000, 16]
        for pinned in (False, True):
            bufs, raw = [], []
            for sz in sizes:
                if pinned:
                    ptr = C.c_void_p()
                    ctx.lib.check(L.sp_host_alloc(C.c_size_t(sz), C.byref(ptr)))
                    raw.append(ptr)
                    bufs.append(np.ctypeslib.as_array((C.c_uint8 * sz).from_address(ptr.value)))
                else:
                    bufs.append(np.zeros(sz, np.uint8))
            bufs[0][:] = src
            p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            rep_c = b._Reply(p(bufs[1]), p(bufs[3]), p(bufs[4]), p(bufs[5]), p(bufs[6]), p(bufs[7]), p(bufs[8]))
            rep_d = b._Reply(None, p(bufs[3]), p(bufs[4]), p(bufs[5]), p(bufs[6]), p(bufs[7]), p(bufs[8]))
            best, chunks = {}, {}
            for leg in ("c", "d", "c", "d") + ("c", "d") * reps:      # two warm-up rounds, then the legs interleaved
                t0 = time.perf_counter()
                if leg == "c":
                    ctx._chk(L.sp_render(ctx.h, C.byref(req), p(bufs[0]), bufs[0].size, width, C.byref(rep_c)))
                else:
                    ctx._chk(L.sp_render_index(ctx.h, C.byref(req), p(bufs[0]), bufs[0].size, width, C.byref(rep_d), p(bufs[2])))
                dt = (time.perf_counter() - t0) * 1e3
                best[leg] = min(best.get(leg, 1e30), dt)
                chunks[leg] = ctx.last_chunks()
            emit({"shape": "host_" + name, "format": fmt, "n": n, "samples": samples, "width": width,
                  "buffers": "page-locked" if pinned else "pageable", "bytes_in": int(src.size), "bytes_out_c": 4 * width * n,
                  "bytes_out_d": width * n, "chunks_c": chunks["c"], "chunks_d": chunks["d"], "c_render_ms": round(best["c"], 3),
                  "d_render_index_ms": round(best["d"], 3), "d_over_c": round(best["d"] / best["c"], 4), "reps": reps})
            del bufs
            for ptr in raw:
                L.sp_host_free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    ctx = pkg.Context(0)
    ctx.enable_timing(True)
    lut = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 3) & 255], axis=1).astype(np.uint8)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    device_legs(pkg, ctx, lut, args.reps, emit)
    if args.host:
        host_legs(pkg, ctx, lut, args.reps, emit)
    ctx.close()


if __name__ == "__main__":
    main()
