"""Whole-reply parity at every launch shape of the frame-loop kernels.

Each case is ONE launch (sp_plan_execute / sp_plan_execute_batch on device-resident operands) whose shape - frames per group, groups
per workgroup, loader, write-out - is chosen with tests/launchref.py for the CU count of the part the test runs on, confirmed through
sp_plan_debug_launch before anything is rendered, and compared whole and bit for bit with the oracle: RGBA bytes, the three gauges,
c_hist, cB_hist and the bit patterns of the dBfs range.  No tolerance.  Inputs are trinoise (every bin of every frame differs) with a
few zeroed frames, one of them in the ragged last group; the LUT is injective; every output buffer starts as garbage and the image
lies between guard bytes that must survive.

k_frames: launchref.frames_lattice() - every (n, gf, loader), every (n, loader, L/R), both layouts and both write-outs at every
(n, gf), the smallest gf in the regimes one / mixed / many and every larger gf at 3 or more groups per workgroup.  sp_geometry admits
requests whose last frame ends past the capture (a byte count that is no multiple of the sample width): two such cases run at 3 or
more groups per workgroup, through the generic loaders.
k_frames_peak: launchref.peak_lattice() against peakref.expected, and the same request forced onto the scratch kernel.
k_frames_batch: launchref.batch_lattice(), every item against the oracle's render of that item.
The last test asserts that every case of the three lattices ran.

The references are computed a few cases ahead on worker threads (the oracle is C behind ctypes), in the order the cases are listed."""
import concurrent.futures as cf

import numpy as np
import pytest

import launchref
import peakref
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 20261, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
ELEM = {"CU4": 1, "CS4": 1, "CU8": 1, "CS8": 1, "CU12": 1, "CS12": 1, "CU16": 2, "CS16": 2, "CU32": 4, "CS32": 4, "CU64": 8, "CS64": 8,
        "CF32": 4, "CF64": 8}
GUARD = 64
MAX_CAPTURE = 128 << 20
TILE = 1000003
GAIN, RANGE = 6.0, 50.0

FRAMES, PEAK, BATCH = launchref.frames_lattice(), launchref.peak_lattice(), launchref.batch_lattice()
RAN = {"frames": set(), "peak": set(), "batch": set()}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _lut():
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    lut[0], lut[-1] = (0, 0, 0), (255, 255, 255)
    assert len({tuple(r) for r in lut.tolist()}) == 256
    return lut


@pytest.fixture(scope="module")
def cu(pkg, ctx):
    """The part's CU count, from the debug entry."""
    win, weight = pyoracle.window("hann", 64)
    plan = ctx.plan("CU8", 64, win, 1.0 / weight, GAIN, RANGE, _lut())
    try:
        return plan.debug_launch(2 * 64 * 4, 4)["cu_count"]
    finally:
        plan.close()


def _trinoise(fmt, samples, seed=0):
    """`samples` samples of trinoise.  Beyond TILE samples the signal repeats: TILE is a prime, so two frames of a capture hold the
    same samples only where their starts differ by a multiple of it - a handful of pairs in the longest captures - and generating
    the longest captures sample by sample would cost more than rendering them."""
    base = siggen.generate(fmt, dict(GEN, seed=GEN["seed"] + seed), min(samples, TILE))
    return base if samples <= TILE else np.resize(base, samples * siggen.SAMPLE_WIDTH[fmt])


def _start(samples_f, n, W, x):
    """worker.js:72, the frame's first sample."""
    return int(0.5 + (samples_f - n) / (W - 1) * x)


def _silence(data, sw, samples_f, n, W, gf):
    """Zeroes a few frames: the second, the middle one and one in the last group."""
    for x in {1, W // 2, W - 1 - ((W - 1) % gf) // 2}:
        s = _start(samples_f, n, W, x)
        data[s * sw:(s + n) * sw] = 0


def _past_its_end(fmt, n, W, samples, seed=0):
    """`samples` samples of trinoise, or a few more, and half a sample behind them: a capture whose last frame ends past it.  The
    frame's start (worker.js:72) is a quotient times W - 1, which at some lengths falls short of the half and rounds down: the first
    length from `samples` on at which it rounds up is taken."""
    sw = siggen.SAMPLE_WIDTH[fmt]
    tail = np.full(ELEM[fmt] * -(-sw // (2 * ELEM[fmt])), 0x5A, np.uint8)
    for more in range(16):
        data = np.concatenate([_trinoise(fmt, samples + more, seed), tail])
        if (_start(data.size / sw, n, W, W - 1) + n) * sw > data.size:
            return data
    raise AssertionError("no capture of %s n=%d W=%d ends inside its last frame" % (fmt, n, W))


def _capture(fmt, n, W, gf, stride, oob=False):
    sw = siggen.SAMPLE_WIDTH[fmt]
    extra = (W - 1) // 3 + 1
    samples = {"overlap": n + (W - 1) * (n // 8) + extra, "exact": n * W, "sparse": n + (W - 1) * (n + n // 2) + extra}[stride]
    if samples * sw > MAX_CAPTURE:
        samples = n + (W - 1) * (n // 8) + extra
    data = _past_its_end(fmt, n, W, samples) if oob else _trinoise(fmt, samples)
    _silence(data, sw, data.size / sw, n, W, gf)
    return data


class _Ahead:
    """make(case) for the cases of a list, a few ahead of the one asked for, on worker threads."""

    def __init__(self, cases, make, depth=6):
        self.cases, self.make, self.depth = cases, make, depth
        self.pool = cf.ThreadPoolExecutor(max_workers=depth)
        self.futures = {}

    def get(self, k):
        for j in range(k, min(k + self.depth, len(self.cases))):
            if j not in self.futures:
                self.futures[j] = self.pool.submit(self.make, self.cases[j])
        return self.futures.pop(k).result()


def _width(c, cu):
    w4 = c["fast"] or c["slow_by"] == "pointer"
    W = launchref.choose_width(c["n"], cu, c["gf"], c["regime"], w4, ragged_group=not (c["gf"] == 4 and w4))
    assert W is not None, "the rule allows no width for %r on %d CUs" % (c, cu)
    return W


def _alloc_reply(ctx, W, n, L, misalign):
    """Device buffers of a reply, all garbage; the image between guards.  -> (pointers for execute(), everything to free, image base)"""
    size = 4 * W * n
    base = ctx.alloc(size + 2 * GUARD + 16)
    ctx.memset(base, 0xAB, size + 2 * GUARD + 16)
    sizes = {"gauge_mins": W, "gauge_maxs": W, "gauge_amps": W, "c_hist": 8 * L, "cb_hist": 8000, "dbfs_minmax": 16}
    ptrs = {k: ctx.alloc(max(v, 16)) for k, v in sizes.items()}
    for k, v in sizes.items():
        ctx.memset(ptrs[k], 0xAB, max(v, 16))
    ptrs["rgba"] = base + GUARD + (4 if misalign else 0)
    assert base % 16 == 0
    return ptrs, base


def _read_reply(ctx, ptrs, base, W, n, L, what):
    size = 4 * W * n
    whole = ctx.download(base, size + 2 * GUARD + 16)
    off = ptrs["rgba"] - base
    assert (whole[:off] == 0xAB).all() and (whole[off + size:] == 0xAB).all(), what + ": bytes around the image were written"
    out = {"rgba": whole[off:off + size]}
    for k in ("gauge_mins", "gauge_maxs", "gauge_amps"):
        out[k] = ctx.download(ptrs[k], W) if W else np.zeros(0, np.uint8)
    out["c_hist"] = ctx.download(ptrs["c_hist"], 8 * L, np.uint64)
    out["cB_hist"] = ctx.download(ptrs["cb_hist"], 8000, np.uint64)
    out["mm"] = ctx.download(ptrs["dbfs_minmax"], 16, np.uint64)
    return out


def _free_reply(ctx, ptrs, base):
    for k, p in ptrs.items():
        if k != "rgba":
            ctx.free(p)
    ctx.free(base)


def _same(got, want, what):
    for k in ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps"):
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero(got[k] != want[k])
            raise AssertionError("%s: %s differs in %d places, first at %d" % (what, k, bad.size, bad[0]))
    assert np.array_equal(got["c_hist"].astype(np.int64), want["c_hist"]), what + ": c_hist differs"
    assert np.array_equal(got["cB_hist"].astype(np.int64), want["cB_hist"]), what + ": cB_hist differs"
    mm = np.array([want["dBfs_min"], want["dBfs_max"]], np.float64).view(np.uint64)
    assert np.array_equal(got["mm"], mm), "%s: dBfs range %r, expected %r" % (what, got["mm"].view(np.float64), mm.view(np.float64))


def _run(ctx, plan, data, W, n, L, misalign, check_launch, what):
    ptrs, base = _alloc_reply(ctx, W, n, L, misalign)
    d_in = ctx.alloc(data.size + 16)
    try:
        check_launch(plan.debug_launch(data.size, W, ptrs["rgba"]))
        ctx.upload(d_in, data)
        plan.execute(d_in, data.size, W, **ptrs)
        ctx.synchronize()
        return _read_reply(ctx, ptrs, base, W, n, L, what)
    finally:
        _free_reply(ctx, ptrs, base)
        ctx.free(d_in)


def _expect_launch(c, cu, kernel, W, M=1):
    def check(d):
        assert d["kernel"] == kernel and d["cu_count"] == cu and d["log2n"] == c["n"].bit_length() - 1, d
        if kernel == "scratch_radix2":
            return
        assert d["gf"] == c["gf"] and d["groups"] == -(-W // c["gf"]) and d["grid"] == launchref.grid_for(d["groups"], cu), d
        assert launchref.regime_of(d["groups"], d["grid"]) == c["regime"], d
        lo, hi = launchref.deal_minmax(d["groups"], d["grid"])
        assert {"one": hi == 1, "mixed": (lo, hi) == (1, 2), "many": lo >= 3}[c["regime"]], (d, lo, hi)
        assert d["prefetch"] == c["loader"] and d["rgba_fast"] == int(c["fast"]) and d["channel_mode"] == int(c["ch"]), d
        assert d["peak_m"] == M and 0 < d["lds_bytes"] <= 160 * 1024, d
        assert d["groups"] % 8 != 0 and (W % c["gf"] != 0 or c["gf"] == 4)
    return check


# ---------------------------------------------------------------------------------------------------------------------- k_frames
@pytest.fixture(scope="module")
def frames_ahead(cu):
    pyoracle.lib()

    def make(c):
        n, W = c["n"], _width(c, cu)
        data = _capture(c["fmt"], n, W, c["gf"], c["stride"], c["oob"])
        win, weight = pyoracle.window("blackmanHarris" if c["wf"] else "hann", n)
        want = pyoracle.render(c["fmt"], data, n, win, 1.0 / weight, GAIN, RANGE, _lut(), W, c["ch"], c["wf"])
        return W, data, win, weight, want

    a = _Ahead(FRAMES, make)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("k", range(len(FRAMES)), ids=[launchref.case_id(c) for c in FRAMES])
def test_k_frames_whole_reply(pkg, ctx, cu, frames_ahead, k):
    c = FRAMES[k]
    what = launchref.case_id(c)
    W, data, win, weight, want = frames_ahead.get(k)
    lut = _lut()
    plan = ctx.plan(c["fmt"], c["n"], win, 1.0 / weight, GAIN, RANGE, lut, c["ch"], c["wf"])
    try:
        got = _run(ctx, plan, data, W, c["n"], len(lut), c["slow_by"] == "pointer", _expect_launch(c, cu, "frames", W), what)
    finally:
        plan.close()
    _same(got, want, "%s W=%d" % (what, W))
    RAN["frames"].add(what)


# ----------------------------------------------------------------------------------------------------------------- k_frames_peak
@pytest.fixture(scope="module")
def peak_ahead(cu):
    pyoracle.lib()

    def make(c):
        n, W, M = c["n"], _width(c, cu), c["M"]
        sw = siggen.SAMPLE_WIDTH[c["fmt"]]
        samples = n + (W - 1) * M * n + (W - 1) // 2 + 1          # a fractional stride: the last column has one sub-frame only
        data = _trinoise(c["fmt"], samples)
        _silence(data, sw, samples, n, W, c["gf"])
        win, weight = pyoracle.window("hann", n)
        want = peakref.expected(c["fmt"], data, n, win, 1.0 / weight, GAIN, RANGE, _lut(), W, c["ch"], c["wf"])
        assert want["M"] == M and want["counts"][-1] < M and all(v == M for v in want["counts"][:-1])
        for key in ("jstar", "counts"):
            want.pop(key)
        return W, data, win, weight, want

    a = _Ahead(PEAK, make, depth=4)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("k", range(len(PEAK)), ids=[launchref.case_id(c) for c in PEAK])
def test_k_frames_peak_whole_reply(pkg, ctx, cu, peak_ahead, k):
    c = PEAK[k]
    what = launchref.case_id(c)
    W, data, win, weight, want = peak_ahead.get(k)
    lut = _lut()
    plan = ctx.plan(c["fmt"], c["n"], win, 1.0 / weight, GAIN, RANGE, lut, c["ch"], c["wf"], detector="peak")
    try:
        for kernel in ("frames_peak", "scratch_radix2"):
            plan.force_kernel("frames" if kernel == "frames_peak" else "scratch")
            got = _run(ctx, plan, data, W, c["n"], len(lut), c["slow_by"] == "pointer", _expect_launch(c, cu, kernel, W, c["M"]), what)
            _same(got, want, "%s W=%d %s" % (what, W, kernel))
    finally:
        plan.close()
    RAN["peak"].add(what)


# ---------------------------------------------------------------------------------------------------------------- k_frames_batch
@pytest.mark.parametrize("k", range(len(BATCH)), ids=[launchref.case_id(c) for c in BATCH])
def test_k_frames_batch_whole_replies(pkg, ctx, cu, k):
    c = BATCH[k]
    what = launchref.case_id(c)
    n, gf, fmt = c["n"], c["gf"], c["fmt"]
    sw = siggen.SAMPLE_WIDTH[fmt]
    widths = launchref.batch_widths(n, gf, cu)
    lut = _lut()
    win, weight = pyoracle.window("hann", n)
    datas = []
    for j, W in enumerate(widths):
        last = j == len(widths) - 1
        if W == 0:
            datas.append(_trinoise(fmt, 3 * n))
        elif W == 1:
            datas.append(_trinoise(fmt, n + 5, j))
        else:
            samples = n + (W - 1) * (n // 4) + (W - 1) // 3 + 1
            # (the last item's last frame ends past the capture: the generic loaders' launch)
            d = _past_its_end(fmt, n, W, samples, j) if last else _trinoise(fmt, samples, j)
            _silence(d, sw, d.size / sw, n, W, gf)
            datas.append(d)
    # the work list the library builds for these shapes: the intended gf, both launches used, the empty item rendered by neither
    pgf, grids, groups, rows = pkg.binding.debug_batch_plan(fmt, n, len(lut), cu, [d.size for d in datas], widths)
    assert pgf == gf == launchref.batch_gf(n, sum(widths), cu)
    # (a single frame of 3-byte samples starts at sample 0: the prefetching loader needs a sample ahead of its last frame)
    assert [int(r[0]) for r in rows] == [1 if sw == 3 else 0, 0, 0, 0, 3, 0, 1], rows
    assert groups[0] + groups[1] >= 3 * cu and grids == (launchref.grid_for(groups[0], cu), launchref.grid_for(groups[1], cu))
    with cf.ThreadPoolExecutor(max_workers=4) as pool:
        wants = list(pool.map(lambda a: pyoracle.render(fmt, a[0], n, win, 1.0 / weight, GAIN, RANGE, lut, a[1], c["ch"], c["wf"]),
                              zip(datas, widths)))
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut, c["ch"], c["wf"])
    held, items = [], []
    try:
        assert plan.debug_launch(datas[-2].size, widths[-2])["kernel"] == "frames"
        for d, W in zip(datas, widths):
            ptrs, base = _alloc_reply(ctx, W, n, len(lut), False)
            d_in = ctx.alloc(d.size + 16)
            ctx.upload(d_in, d)
            held.append((ptrs, base, d_in))
            items.append((d_in, d.size, W, ptrs))
        plan.execute_batch(items)
        ctx.synchronize()
        for j, ((ptrs, base, d_in), W) in enumerate(zip(held, widths)):
            _same(_read_reply(ctx, ptrs, base, W, n, len(lut), what), wants[j], "%s item %d W=%d" % (what, j, W))
    finally:
        for ptrs, base, d_in in held:
            _free_reply(ctx, ptrs, base)
            ctx.free(d_in)
        plan.close()
    RAN["batch"].add(what)


# ------------------------------------------------------------------------------------------------------------------ completeness
def test_zz_the_whole_lattice_ran(cu):
    """Runs last in the module: every case launchref enumerates has run (and passed) on this part, none skipped but the cells the rule
    puts out of reach at this CU count (launchref.unreachable_by_rule: none of the lattices' cells on 16 CUs or on 24 and more)."""
    for name, cases in (("frames", FRAMES), ("peak", PEAK), ("batch", BATCH)):
        assert len({launchref.case_id(c) for c in cases}) == len(cases)
        ids = {launchref.case_id(c) for c in (cases if name == "batch" else launchref.reachable(cases, cu))}
        assert RAN[name] == ids, "%s: %d of %d cases ran on %d CUs; missing %s" % (name, len(RAN[name]), len(ids), cu, sorted(ids - RAN[name])[:8])
    assert {(c["n"], c["gf"]) for c in FRAMES} == set(launchref.gf_pairs())
