#!/usr/bin/env python3
"""Batches of small captures: K consecutive sp_plan_execute calls against one sp_plan_execute_batch of the same K items (device-resident
captures from sp_synth_trinoise), and the host path: K sp_render calls against one sp_render_batch.

Two shapes: config-1 items (cu8, n = 512, 2^20 samples, width 2 048) and thumbnail items (cu8, n = 256, 256 KiB, width 256), K in
{1, 8, 64, 256}.  Device times come from HIP events on the context's stream (best of --reps after a warm-up); the host path is timed by
the host clock (best of --reps after a warm-up).  Per case: us per item, frames/s, the fraction of the 8 TB/s HBM roofline (sw * min(stride, n) + 4n + 3
bytes per frame) and a checksum of every output of (a) and of (b), which must agree.  For kernel durations without the event pairs, run
it under `rocprofv3 --kernel-trace --stats -- python tools/batch_bench.py` (kernels k_frames, k_frames_batch, k_batch_clear).
Prints one JSON line per case."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SHAPES = {"config1": dict(fmt="cu8", n=512, samples=1 << 20, width=2048),
          "thumb": dict(fmt="cu8", n=256, samples=(256 << 10) // 2, width=256)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--shapes", default="config1,thumb")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    ctx.set_stream(stream.cuda_stream)
    for shape in args.shapes.split(","):
        s = SHAPES[shape]
        fmt, n, S, W = s["fmt"], s["n"], s["samples"], s["width"]
        sw = 2
        win, weight = pkg.window("blackmanHarris", n)
        i = np.arange(256)
        lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
        lut[0], lut[-1] = 0, 255
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
        stride = (S - n) / (W - 1)
        bpf = sw * min(stride, n) + 4 * n + 3
        for K in [int(k) for k in args.ks.split(",")]:
            nbytes = S * sw
            d_in = ctx.alloc(K * nbytes)
            ctx.synth_trinoise(d_in, fmt, 0, K * S, 4242, 7321, 11, 0.5, 0.02)
            img_b, rec_b = 4 * W * n, 8 * (256 + 1000) + 16 + 3 * W
            outs = {}
            for mode in ("single", "batch"):
                d_img, d_rec = ctx.alloc(K * img_b), ctx.alloc(K * rec_b)
                ctx.memset(d_img, 0x5A, K * img_b)
                items = []
                for k in range(K):
                    r = d_rec + k * rec_b
                    o = {"rgba": d_img + k * img_b, "c_hist": r, "cb_hist": r + 2048, "dbfs_minmax": r + 10048,
                         "gauge_mins": r + 10064, "gauge_maxs": r + 10064 + W, "gauge_amps": r + 10064 + 2 * W}
                    items.append((d_in + k * nbytes, nbytes, W, o))

                def run():
                    if mode == "batch":
                        plan.execute_batch(items)
                    else:
                        for it in items:
                            plan.execute(it[0], it[1], it[2], **it[3])
                run()
                stream.synchronize()
                best = 1e30
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    run()
                    e1.record(stream)
                    e1.synchronize()
                    best = min(best, e0.elapsed_time(e1) * 1e3)
                h = hashlib.sha256()
                h.update(ctx.download(d_img, K * img_b).tobytes())
                h.update(ctx.download(d_rec, K * rec_b).tobytes())
                outs[mode] = (best, h.hexdigest()[:16])
                ctx.free(d_img)
                ctx.free(d_rec)
            # (c) the host path: best of --reps after one warm-up call of each
            host = [ctx.download(d_in + k * nbytes, nbytes) for k in range(K)]

            def singles():
                for d in host:
                    ctx.render(fmt, d, n, win, 1.0 / weight, 6.0, 30.0, lut, W)

            def batched():
                ctx.render_batch(fmt, host, n, win, 1.0 / weight, 6.0, 30.0, lut, [W] * K)

            t_single_host = t_batch_host = 1e30
            singles()
            batched()
            for _ in range(args.reps):
                t0 = time.perf_counter()
                singles()
                t_single_host = min(t_single_host, (time.perf_counter() - t0) * 1e6)
                t0 = time.perf_counter()
                batched()
                t_batch_host = min(t_batch_host, (time.perf_counter() - t0) * 1e6)
            ctx.free(d_in)
            frames = K * W
            rec = {"shape": shape, "K": K, "n": n, "width": W,
                   "a_single_us_per_item": round(outs["single"][0] / K, 2), "b_batch_us_per_item": round(outs["batch"][0] / K, 2),
                   "speedup_b_over_a": round(outs["single"][0] / outs["batch"][0], 2),
                   "a_frames_per_s": round(frames / outs["single"][0] * 1e6), "b_frames_per_s": round(frames / outs["batch"][0] * 1e6),
                   "a_roofline": round(frames * bpf / (outs["single"][0] * 1e-6) / 8e12, 4),
                   "b_roofline": round(frames * bpf / (outs["batch"][0] * 1e-6) / 8e12, 4),
                   "checksum_a": outs["single"][1], "checksum_b": outs["batch"][1], "same": outs["single"][1] == outs["batch"][1],
                   "c_render_us_per_item": round(t_single_host / K, 1), "c_render_batch_us_per_item": round(t_batch_host / K, 1)}
            print(json.dumps(rec), flush=True)
        plan.close()
    ctx.set_stream(0)
    ctx.close()


if __name__ == "__main__":
    main()
