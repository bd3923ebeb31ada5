"""Soak run (not collected by pytest; run by hand on the GPU box): many more seeded random requests than the suite holds, plus
long large-n requests (n = 2048 .. 8192, up to 700 frames: many groups per workgroup, partial last groups) and, as ONE launch each
(sp_plan_execute), wide requests chosen with tests/launchref.py so that every frames-per-group value of every n is reached at three
or more groups per workgroup on the part at hand, every output bit-exact against the C oracle.
    python3 tests/soak_gpu.py [cases] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle
import launchref
from test_gpu_parity import _random_cases


def big_cases(count, seed):
    rs = np.random.RandomState(seed)
    fmts = ["CU8", "CS8", "CU12", "CS12", "CU16", "CS16", "CF32", "CS32", "CF64"]
    out = []
    for _ in range(count):
        n = int(rs.choice([1024, 2048, 2048, 4096, 8192]))
        frames = int(rs.randint(100, 700))
        hop = max(1, n // int(rs.choice([1, 1, 2, 4, 8])))
        samples = n + (frames - 1) * hop + int(rs.randint(0, 5))
        out.append(dict(fmt=str(rs.choice(fmts)), n=n, width=frames, samples=samples, win="hann", gain=float(rs.randint(0, 40)),
                        rng=float(rs.choice([30, 60, 90])), ch=bool(rs.randint(4) == 0), wf=bool(rs.randint(4) == 0), lut_len=256,
                        seed=int(rs.randint(1 << 30)), amp=float(rs.choice([0.05, 0.5])), kind="trinoise"))
    return out


def wide_cases(cu, seed):
    """One request per (n, frames per group) at 3 or more groups per workgroup; format, layout, split and raggedness by seed."""
    rs = np.random.RandomState(seed)
    fmts = ["CU4", "CU8", "CS8", "CS12", "CS16", "CF32", "CS32", "CF64"]
    out = []
    for n, gf in launchref.gf_pairs():
        w4 = bool(rs.randint(2))
        width = launchref.choose_width(n, cu, gf, "many", w4, ragged_group=not (gf == 4 and w4))
        hop = max(1, n // int(rs.choice([4, 8, 16])))
        out.append(dict(fmt=str(rs.choice(fmts)), n=n, width=width, samples=n + (width - 1) * hop + int(rs.randint(0, width)), win="hann",
                        gain=float(rs.randint(0, 40)), rng=float(rs.choice([30, 60, 90])), ch=bool(rs.randint(4) == 0), wf=bool(rs.randint(4) == 0),
                        lut_len=256, seed=int(rs.randint(1 << 30)), amp=float(rs.choice([0.05, 0.5])), kind="trinoise", gf=gf, one_launch=True))
    return out


def render_one_launch(ctx, c, data, win, weight, lut):
    """The request through sp_plan_execute on device buffers: one launch, its frames per group confirmed by sp_plan_debug_launch."""
    n, W, L = c["n"], c["width"], len(lut)
    plan = ctx.plan(c["fmt"], n, win, 1.0 / weight, c["gain"], c["rng"], lut, c["ch"], c["wf"])
    sizes = {"rgba": 4 * W * n, "gauge_mins": W, "gauge_maxs": W, "gauge_amps": W, "c_hist": 8 * L, "cb_hist": 8000, "dbfs_minmax": 16}
    ptrs = {k: ctx.alloc(v) for k, v in sizes.items()}
    d_in = ctx.alloc(data.size)
    try:
        d = plan.debug_launch(data.size, W, ptrs["rgba"])
        assert d["kernel"] == "frames" and d["gf"] == c["gf"] and min(launchref.deal(d["groups"], d["grid"])) >= 3, d
        ctx.upload(d_in, data)
        plan.execute(d_in, data.size, W, **ptrs)
        ctx.synchronize()
        got = {k: ctx.download(ptrs[k], sizes[k]) for k in ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps")}
        got["c_hist"] = ctx.download(ptrs["c_hist"], 8 * L, np.uint64)
        got["cB_hist"] = ctx.download(ptrs["cb_hist"], 8000, np.uint64)
        got["dBfs_min"], got["dBfs_max"] = ctx.download(ptrs["dbfs_minmax"], 16, np.float64)
        return got
    finally:
        for p in list(ptrs.values()) + [d_in]:
            ctx.free(p)
        plan.close()


def check(ctx, c):
    kind = c["kind"] if not c["fmt"].startswith("CF") else "trinoise"
    gen = {"kind": kind, "seed": c["seed"], "step": 4099, "gshift": 9, "amp": c["amp"], "namp": 0.02}
    data = siggen.generate(c["fmt"], gen, c["samples"])
    win, weight = pyoracle.window(c["win"], c["n"])
    if weight == 0:          # hann / bartlett / blackman at n = 2: an all-zero taper
        return []
    i = np.arange(c["lut_len"])
    lut = np.stack([(i * 5) & 255, (i * 11 + 3) & 255, (255 - i) & 255], axis=1).astype(np.uint8)
    want = pyoracle.render(c["fmt"], data, c["n"], win, 1.0 / weight, c["gain"], c["rng"], lut, c["width"], c["ch"], c["wf"])
    if c.get("one_launch"):
        got = render_one_launch(ctx, c, data, win, weight, lut)
    else:
        got = ctx.render(c["fmt"], data, c["n"], win, 1.0 / weight, c["gain"], c["rng"], lut, c["width"], c["ch"], c["wf"])
    bad = [k for k in ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps") if not np.array_equal(got[k], want[k])]
    bad += [k for k in ("c_hist", "cB_hist") if not np.array_equal(got[k].astype(np.int64), want[k])]
    for k in ("dBfs_min", "dBfs_max"):
        a, b = np.float64(got[k]), np.float64(want[k])
        if not ((a != a and b != b) or a.view(np.uint64) == b.view(np.uint64)):
            bad.append(k)
    return bad


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    pkg = load_package()
    ctx = pkg.Context(0)
    win, weight = pyoracle.window("hann", 64)
    probe = ctx.plan("CU8", 64, win, 1.0 / weight, 0.0, 30.0, np.zeros((2, 3), np.uint8))
    cu = probe.debug_launch(1024, 4)["cu_count"]
    probe.close()
    wide = wide_cases(cu, seed + 2)
    cases = _random_cases(count, seed) + big_cases(max(1, count // 8), seed + 1) + wide
    failed = 0
    for k, c in enumerate(cases):
        bad = check(ctx, c)
        if bad:
            failed += 1
            print("MISMATCH", bad, c, flush=True)
    print("soak: %d cases (%d long large-n, %d wide single launches on %d CUs), %d mismatches, seed %d"
          % (len(cases), max(1, count // 8), len(wide), cu, failed, seed))
    ctx.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
