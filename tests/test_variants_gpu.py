"""Every compiled variant of the frame-loop kernels launched once and compared whole with the oracle.

One case per cell of tests/variantref.py's lattice (tests/test_variants_cpu.py pins it against the built objects: 417 kernels).  Each
case shapes its launch for 8 CUs (Context.set_cu_count, put back in a finally): the smallest frames per group of its n, 19 groups with a
ragged last one, frames that overlap with a stride of n / 2 + 3 samples.  Before anything is compared the case asserts which variant
serves it - kernel, log2n, channel mode and loader from sp_plan_debug_launch / sp_plan_debug_index_launch, the traces' and the power
plane's kernel from their kernel_name_for next to the plan's launch (they call frames_prefetch_width on the same request), a batch's two
launches from sp_debug_batch_plan - so that a fall-back to the scratch kernels or to render_extract fails the case.  Every comparison is
bit for bit, no tolerance:
    frames  sp_plan_execute against pyoracle.render, every reply field
    batch   three items (gf + 1 frames, 1 frame, the rest) in one sp_plan_execute_batch, each against the oracle
    peak    a sparse capture, M = 2 or 3 sub-frames per column, against peakref
    traces  against tracesref;  power: against powerref, whose plane must be telling;  index: the oracle's image through indexref
Inputs, garbage-filled outputs and guard bytes are those of tests/test_launch_shapes_gpu.py.  The last test asserts that every cell ran."""
import time

import numpy as np
import pytest

import launchref
import peakref
import powerref
import siggen
import test_index_launch_shapes_gpu as shapes
import test_launch_shapes_gpu as base
import test_scratch_shapes_gpu as ss
import tracesref
import variantref
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GAIN, RANGE = base.GAIN, base.RANGE
CU = variantref.CU
CELLS = variantref.lattice()
IDS = [variantref.case_id(c) for c in CELLS]
RAN = set()
TIMES = {}

pkg = base.pkg


@pytest.fixture(scope="module")
def ctx(pkg):
    """The module's own context: no other module sees the override."""
    c = pkg.Context(0)
    yield c
    c.set_cu_count(0)
    c.close()


def _reported(ctx):
    win, weight = pyoracle.window("hann", 64)
    plan = ctx.plan("CU8", 64, win, 1.0 / weight, GAIN, RANGE, base._lut())
    try:
        return plan.debug_launch(2 * 64 * 4, 4)["cu_count"]
    finally:
        plan.close()


@pytest.fixture(scope="module")
def own(ctx):
    ctx.set_cu_count(0)
    return _reported(ctx)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


NOISY = dict(base.GEN, amp=0.35, namp=0.3)      # 4-bit samples: with base.GEN's 0.2 LSB of noise a short frame has bins that are exactly zero


def _capture(c, W, samples, seed=0, silence=True):
    if c["loader"] == 1:
        data = siggen.generate(c["fmt"], dict(NOISY, seed=NOISY["seed"] + seed), samples)
    else:
        data = base._trinoise(c["fmt"], samples, seed)
    if silence and W > 1:
        base._silence(data, siggen.SAMPLE_WIDTH[c["fmt"]], samples, c["n"], W, variantref.gf_of(c["n"]))
    return data


def _make(c):
    """The capture(s), the taper and the reference of a cell."""
    n, family, lut = c["n"], c["family"], base._lut()
    win, weight = pyoracle.window("blackmanHarris" if c["wf"] else "hann", n)
    bn = 1.0 / weight
    reqs = variantref.requests(c)
    if family == "batch":
        datas = [_capture(c, W, samples, j) for j, (W, samples, _) in enumerate(reqs)]
        wants = [pyoracle.render(c["fmt"], d, n, win, bn, GAIN, RANGE, lut, W, c["ch"], c["wf"]) for d, (W, _, _) in zip(datas, reqs)]
        return datas, win, bn, wants
    (W, samples, nbytes), = reqs
    data = _capture(c, W, samples, silence=family != "power")
    assert data.size == nbytes
    if family in ("frames", "index"):
        want = pyoracle.render(c["fmt"], data, n, win, bn, GAIN, RANGE, lut, W, c["ch"], c["wf"])
    elif family == "peak":
        want = peakref.expected(c["fmt"], data, n, win, bn, GAIN, RANGE, lut, W, c["ch"], c["wf"])
        assert want["M"] == c["M"] and want["counts"][-1] == 1 and all(v == c["M"] for v in want["counts"][:-1])
        want = {k: v for k, v in want.items() if k not in ("jstar", "counts", "M")}
    elif family == "traces":
        want = tracesref.expected(c["fmt"], data, n, win, bn, GAIN, RANGE, W, c["ch"])
    else:
        want = powerref.expected(c["fmt"], data, n, win, bn, GAIN, RANGE, W, c["ch"])["power"]
        powerref.assert_telling(want[:, 1:] if c["ch"] else want, variantref.case_id(c))      # (row 0 of an L/R split is bin n / 2: zero)
    return data, win, bn, want


@pytest.fixture(scope="module")
def ahead():
    pyoracle.lib()
    a = base._Ahead(CELLS, _make, depth=6)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


def _is_cell(c, d, kernel, W):
    """The launch sp_plan_debug_launch / sp_plan_debug_index_launch reports is the cell's variant at the cell's shape."""
    assert d["kernel"] == kernel and d["cu_count"] == CU, d
    assert (d["log2n"], d["channel_mode"], d["prefetch"]) == (c["n"].bit_length() - 1, int(c["ch"]), c["loader"]), d
    assert (d["gf"], d["groups"], d["grid"]) == (variantref.gf_of(c["n"]), variantref.GROUPS, 8) and W % d["gf"] != 0, d
    assert 0 < d["lds_bytes"] <= 160 * 1024, d


def _image(ctx, plan, c, data, W, want, what):
    n, lut, family = c["n"], base._lut(), c["family"]

    def check(d):
        _is_cell(c, d, {"frames": "frames", "peak": "frames_peak", "index": "frames_index"}[family], W)
        assert d["rgba_fast"] == int(variantref.is_fast(c)), d
        if family == "peak":
            assert d["peak_m"] == c["M"], d

    if family == "index":
        assert plan.index_kernel_name_for(data.size, W) == "frames_index"
        got = shapes.run(ctx, plan, data, W, n, len(lut), 0, check, what)
        shapes.same(got, want, what)
    else:
        got = base._run(ctx, plan, data, W, n, len(lut), False, check, what)
        base._same(got, want, what)


def _plane(ctx, plan, c, data, W, want, what):
    n, family = c["n"], c["family"]
    _is_cell(c, plan.debug_launch(data.size, W), "frames", W)
    d_in = ctx.alloc(data.size + 16)
    outs = [ss._Dev(ctx, 8 * n), ss._Dev(ctx, 8 * n)] if family == "traces" else [ss._Dev(ctx, 8 * W * n)]
    try:
        ctx.upload(d_in, data)
        if family == "traces":
            assert plan.traces_kernel_name_for(data.size, W) == "frames_traces"
            plan.execute_traces(d_in, data.size, W, outs[0].ptr, outs[1].ptr)
            ctx.synchronize()
            got = {"trace_min": outs[0].read(np.float64, what), "trace_max": outs[1].read(np.float64, what)}
        else:
            assert plan.power_kernel_name_for(data.size, W) == "frames_power"
            plan.execute_power(d_in, data.size, W, outs[0].ptr)
            ctx.synchronize()
            got = outs[0].read(np.float64, what).reshape(W, n)
    finally:
        for o in outs:
            o.free()
        ctx.free(d_in)
    if family == "traces":
        tracesref.assert_same(got, want, what)
    else:
        powerref.assert_same(got, want, what)


def _batch(pkg, ctx, plan, c, datas, wants, what):
    n, lut, gf = c["n"], base._lut(), variantref.gf_of(c["n"])
    widths = [W for W, _, _ in variantref.requests(c)]
    pgf, grids, groups, rows = pkg.binding.debug_batch_plan(c["fmt"], n, len(lut), CU, [d.size for d in datas], widths)
    assert pgf == gf and [int(r[0]) for r in rows] == variantref.batch_launches(c) and sum(groups) == variantref.GROUPS, (what, rows)
    mine = 1 if c["loader"] == 0 else 0                       # the launch of the cell's variant: the one that holds the ragged large item
    assert int(rows[2][0]) == mine and groups[mine] >= variantref.GROUPS - 3 and grids[mine] == 8, (what, rows, groups, grids)
    d = plan.debug_launch(datas[2].size, widths[2])          # the format's loader for an item of this kind, the plan's n and channel mode
    assert (d["kernel"], d["log2n"], d["channel_mode"], d["prefetch"], d["cu_count"]) == ("frames", n.bit_length() - 1, int(c["ch"]), c["loader"], CU), d
    held, items = [], []
    try:
        for dj, W in zip(datas, widths):
            ptrs, blk = base._alloc_reply(ctx, W, n, len(lut), False)
            d_in = ctx.alloc(dj.size + 16)
            ctx.upload(d_in, dj)
            held.append((ptrs, blk, d_in))
            items.append((d_in, dj.size, W, ptrs))
        plan.execute_batch(items)
        ctx.synchronize()
        for j, ((ptrs, blk, _), W) in enumerate(zip(held, widths)):
            base._same(base._read_reply(ctx, ptrs, blk, W, n, len(lut), what), wants[j], "%s item %d W=%d" % (what, j, W))
    finally:
        for ptrs, blk, d_in in held:
            base._free_reply(ctx, ptrs, blk)
            ctx.free(d_in)


@pytest.mark.parametrize("k", range(len(CELLS)), ids=IDS)
def test_variant_whole_reply(pkg, ctx, ahead, k):
    c = CELLS[k]
    what, family = IDS[k], c["family"]
    data, win, bn, want = ahead.get(k)
    plan = ctx.plan(c["fmt"], c["n"], win, bn, GAIN, RANGE, base._lut(), c["ch"], c["wf"], detector="peak" if family == "peak" else "sample")
    try:
        ctx.set_cu_count(CU)
        if family == "batch":
            _batch(pkg, ctx, plan, c, data, want, what)
        elif family in ("traces", "power"):
            _plane(ctx, plan, c, data, variantref.width_of(c), want, what)
        else:
            _image(ctx, plan, c, data, variantref.width_of(c), want, what)
    finally:
        ctx.set_cu_count(0)
        plan.close()
    RAN.add(what)


def test_zz_every_case_ran(ctx, own):
    """Runs last in the module: every cell of the lattice ran (and passed), no override is left behind.  Prints the module's case
    count, total time and slowest case."""
    assert len(set(IDS)) == len(IDS) == 417
    assert RAN == set(IDS), "%d of %d cases ran; missing %s" % (len(RAN), len(IDS), sorted(set(IDS) - RAN)[:8])
    assert _reported(ctx) == own
    slowest = max(TIMES, key=TIMES.get)
    print("\ntest_variants_gpu: %d cases, %.1f s in all, slowest %s %.2f s" % (len(TIMES), sum(TIMES.values()), slowest, TIMES[slowest]))
