"""Every format's capture tail through every kernel family, whole replies against the oracle, bit for bit.

The cases are those of tests/tailref.py (tests/test_tails_cpu.py proves on the oracle that each is telling and pins the oracle's decode
of all 32 (format, tail) pairs to the reference's): every (format, tail) in the regimes `overhang` and `short`
    - through k_frames, k_frames_peak, k_frames_traces, k_frames_power and k_frames_index, n alternating between 64 and 1024, host-fed
      (Context.render*) or device-resident (Plan.execute*), the L/R split and the layout rotating;
    - as the items of one batch per format (n = 64 or 512) next to an item of whole samples;
    - through the scratch kernels at n = 32 and n = 2048 (forced), image, peak, traces and power.
A device-resident capture lies between two guards of 0x5A, n sample widths or more each: a loader that ignores a bound reads guard bytes
and the comparison fails; nothing faults.  A host-fed capture lies in a host array between the same guards.  Of a device-resident case the
served kernel and its loader are asserted before anything is compared: the generic loaders (prefetch == 0) wherever a frame leaves the
capture, the format's prefetching loader where the capture ends flush with its last frame (a tail under half a sample cannot overhang:
tailref).  Byte counts the reference throws on are refused with status -3 by every entry point.  The last test asserts that every case ran."""
import time

import numpy as np
import pytest

import indexref
import peakref
import powerref
import siggen
import tailref
import test_index_launch_shapes_gpu as shapes
import test_launch_shapes_gpu as base
import test_scratch_shapes_gpu as ss
import tracesref
import variantref
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GAIN, RANGE = base.GAIN, base.RANGE
CASES, SCRATCH, BATCHES = tailref.lattice(), tailref.scratch_lattice(), tailref.batches()
ALL = CASES + SCRATCH
IDS = [tailref.case_id(c) for c in ALL]
BATCH_IDS = [tailref.case_id(b) for b in BATCHES]
RAN = set()
TIMES = {}

pkg, ctx, cu = base.pkg, base.ctx, base.cu   # (module-scoped fixtures, instantiated for this module)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


def _kind(c):
    return c.get("kind", {"frames": "image"}.get(c["family"], c["family"]))


def _taper(n):
    win, weight = pyoracle.window(tailref.WINDOW, n)
    return win, 1.0 / weight


def _reference(kind, fmt, data, n, W, ch, wf):
    win, bn = _taper(n)
    lut = base._lut()
    if kind in ("image", "index"):
        return pyoracle.render(fmt, data, n, win, bn, GAIN, RANGE, lut, W, ch, wf)
    if kind == "peak":
        want = peakref.expected(fmt, data, n, win, bn, GAIN, RANGE, lut, W, ch, wf)
        return {k: v for k, v in want.items() if k not in ("jstar", "counts")}
    if kind == "traces":
        return tracesref.expected(fmt, data, n, win, bn, GAIN, RANGE, W, ch)
    return powerref.expected(fmt, data, n, win, bn, GAIN, RANGE, W, ch)["power"]


def _make(c):
    W, data = tailref.request(c)
    return W, data, _reference(_kind(c), c["fmt"], data, c["n"], W, c["ch"], c["wf"])


@pytest.fixture(scope="module")
def ahead():
    pyoracle.lib()
    a = base._Ahead(ALL, _make, depth=6)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


class _Capture:
    """A capture on the device between its guards."""

    def __init__(self, ctx, fmt, n, data):
        G, g = tailref.guarded(fmt, n, data)
        self.ctx, self.blk = ctx, ctx.alloc(G.size)
        assert self.blk % 16 == 0 and g % 16 == 0
        ctx.upload(self.blk, G)
        self.ptr, self.nbytes = self.blk + g, data.size

    def free(self):
        self.ctx.free(self.blk)


def _host_view(fmt, n, data):
    """The capture as a view into a host array that holds the guards around it."""
    G, g = tailref.guarded(fmt, n, data)
    v = G[g:g + data.size]
    assert v.flags["C_CONTIGUOUS"] and v.base is G
    return v


def _same_host(got, want, what):
    """A host-fed reply (binding.Context.render's dict) against the oracle's, the dBfs range by its bits."""
    if "index" in got:
        assert np.array_equal(got["index"], indexref.expected_index(want)), what + ": index differs"
    else:
        assert np.array_equal(got["rgba"], want["rgba"]), what + ": rgba differs in %d places" % np.count_nonzero(got["rgba"] != want["rgba"])
    for k in ("gauge_mins", "gauge_maxs", "gauge_amps"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)
    assert np.array_equal(got["c_hist"].astype(np.int64), want["c_hist"]) and np.array_equal(got["cB_hist"].astype(np.int64), want["cB_hist"]), what
    mm = lambda r: np.array([r["dBfs_min"], r["dBfs_max"]], np.float64).view(np.uint64)
    assert np.array_equal(mm(got), mm(want)), "%s: dBfs range %r %r" % (what, got["dBfs_min"], got["dBfs_max"])


def _expect_loader(c, nbytes, W):
    """The loader of the frame-loop launch: 0 wherever a frame leaves the capture."""
    p = variantref.prefetch_width(c["fmt"], c["n"], nbytes, W)
    if tailref.leaving(c["fmt"], c["n"], nbytes, W):
        assert p == 0
    return p


def _host_fed(ctx, c, W, data, want, what):
    kind, n, fmt = _kind(c), c["n"], c["fmt"]
    win, bn = _taper(n)
    view = _host_view(fmt, n, data)
    if kind in ("image", "peak"):
        _same_host(ctx.render(fmt, view, n, win, bn, GAIN, RANGE, base._lut(), W, c["ch"], c["wf"], detector="peak" if kind == "peak" else "sample"), want, what)
    elif kind == "index":
        _same_host(ctx.render_index(fmt, view, n, win, bn, GAIN, RANGE, base._lut(), W, c["ch"], c["wf"], fill=0xAB), want, what)
    elif kind == "traces":
        tracesref.assert_same(ctx.render_traces(fmt, view, n, win, bn, GAIN, RANGE, W, c["ch"], fill=7.0), want, what)
    else:
        powerref.assert_same(ctx.render_power(fmt, view, n, win, bn, GAIN, RANGE, W, c["ch"], fill=0xAB), want, what)


def _resident(ctx, c, W, data, want, what):
    kind, n, fmt, lut = _kind(c), c["n"], c["fmt"], base._lut()
    scratch = c["family"].startswith("scratch")
    win, bn = _taper(n)
    plan = ctx.plan(fmt, n, win, bn, GAIN, RANGE, lut, c["ch"], c["wf"], detector="peak" if kind == "peak" else "sample")
    cap = _Capture(ctx, fmt, n, data)
    nb = cap.nbytes
    try:
        if scratch and n >= 64:
            plan.force_kernel("scratch")
        M = want.pop("M") if kind == "peak" else 1
        d = plan.debug_launch(nb, W)
        assert d["log2n"] == n.bit_length() - 1 and d["channel_mode"] == int(c["ch"]) and d["peak_m"] == M, (what, d)
        if scratch:
            assert d["kernel"] == "scratch_radix2", (what, d)
        else:
            assert d["kernel"] == ("frames_peak" if M >= 2 else "frames") and d["prefetch"] == _expect_loader(c, nb, W), (what, d)
        if kind in ("image", "peak"):
            ptrs, blk = base._alloc_reply(ctx, W, n, len(lut), False)
            try:
                plan.execute(cap.ptr, nb, W, **ptrs)
                ctx.synchronize()
                got = base._read_reply(ctx, ptrs, blk, W, n, len(lut), what)
            finally:
                base._free_reply(ctx, ptrs, blk)
            base._same(got, want, what)
        elif kind == "index":
            ptrs, blk = shapes._alloc(ctx, W, n, len(lut), 0)
            try:
                di = plan.debug_index_launch(nb, W, ptrs["index"])
                assert plan.index_kernel_name_for(nb, W) == "frames_index" and di["kernel"] == "frames_index", (what, di)
                assert di["prefetch"] == _expect_loader(c, nb, W) and di["channel_mode"] == int(c["ch"]), (what, di)
                plan.execute_index(cap.ptr, nb, W, **ptrs)
                ctx.synchronize()
                got = shapes._read(ctx, ptrs, blk, W, n, len(lut), what)
            finally:
                shapes._free(ctx, ptrs, blk)
            shapes.same(got, want, what)
        elif kind == "traces":
            assert plan.traces_kernel_name_for(nb, W) == ("scratch_traces" if scratch else "frames_traces"), what
            lo, hi = ss._Dev(ctx, 8 * n), ss._Dev(ctx, 8 * n)
            try:
                plan.execute_traces(cap.ptr, nb, W, lo.ptr, hi.ptr)
                ctx.synchronize()
                got = {"trace_min": lo.read(np.float64, what), "trace_max": hi.read(np.float64, what)}
            finally:
                lo.free()
                hi.free()
            tracesref.assert_same(got, want, what)
        else:
            assert plan.power_kernel_name_for(nb, W) == ("scratch_power" if scratch else "frames_power"), what
            pl = ss._Dev(ctx, 8 * W * n)
            try:
                plan.execute_power(cap.ptr, nb, W, pl.ptr)
                ctx.synchronize()
                got = pl.read(np.float64, what).reshape(W, n)
            finally:
                pl.free()
            powerref.assert_same(got, want, what)
    finally:
        cap.free()
        plan.close()


@pytest.mark.parametrize("k", range(len(ALL)), ids=IDS)
def test_tail_whole_reply(ctx, ahead, k):
    c, what = ALL[k], IDS[k]
    W, data, want = ahead.get(k)
    if c["host"]:
        if _kind(c) == "peak":
            want.pop("M")
        _host_fed(ctx, c, W, data, want, what)
    else:
        _resident(ctx, c, W, data, want, what)
    RAN.add(what)


@pytest.mark.parametrize("k", range(len(BATCHES)), ids=BATCH_IDS)
def test_tail_batch_whole_replies(pkg, ctx, cu, k):
    """One batch per format: every tail in both regimes as an item - the generic launch wherever a frame leaves the capture - and an item
    of whole samples for the prefetching launch."""
    b, what = BATCHES[k], BATCH_IDS[k]
    fmt, n, lut = b["fmt"], b["n"], base._lut()
    win, bn = _taper(n)
    reqs = [tailref.request(it, seed=j) for j, it in enumerate(b["items"])] + [tailref.whole_item(fmt, n)]
    widths, datas = [W for W, _ in reqs], [d for _, d in reqs]
    wants = [pyoracle.render(fmt, d, n, win, bn, GAIN, RANGE, lut, W, b["ch"], b["wf"]) for W, d in reqs]
    if b["host"]:
        gots = ctx.render_batch(fmt, [_host_view(fmt, n, d) for d in datas], n, win, bn, GAIN, RANGE, lut, widths, b["ch"], b["wf"])
        for j, (g, w) in enumerate(zip(gots, wants)):
            _same_host(g, w, "%s item %d" % (what, j))
        RAN.add(what)
        return
    pgf, grids, groups, rows = pkg.binding.debug_batch_plan(fmt, n, len(lut), cu, [d.size for d in datas], widths)
    launches = [int(r[0]) for r in rows]
    for j, (W, d) in enumerate(reqs):
        out = tailref.leaving(fmt, n, d.size, W)
        assert launches[j] == (0 if variantref.prefetch_width(fmt, n, d.size, W) else 1) and (launches[j] == 1 or not out), (what, j, rows)
    assert launches[-1] == (1 if siggen.SAMPLE_WIDTH[fmt] == 16 else 0) and launches.count(1) >= len(b["items"]) // 2, (what, launches)
    plan = ctx.plan(fmt, n, win, bn, GAIN, RANGE, lut, b["ch"], b["wf"])
    held, items = [], []
    try:
        assert plan.debug_launch(datas[-1].size, widths[-1])["kernel"] == "frames"
        for d, W in zip(datas, widths):
            ptrs, blk = base._alloc_reply(ctx, W, n, len(lut), False)
            cap = _Capture(ctx, fmt, n, d)
            held.append((ptrs, blk, cap))
            items.append((cap.ptr, d.size, W, ptrs))
        plan.execute_batch(items)
        ctx.synchronize()
        for j, ((ptrs, blk, _), W) in enumerate(zip(held, widths)):
            base._same(base._read_reply(ctx, ptrs, blk, W, n, len(lut), what), wants[j], "%s item %d W=%d" % (what, j, W))
    finally:
        for ptrs, blk, cap in held:
            base._free_reply(ctx, ptrs, blk)
            cap.free()
        plan.close()
    RAN.add(what)


@pytest.mark.parametrize("fmt,tail", tailref.REFUSED, ids=["%s+%d" % p for p in tailref.REFUSED])
def test_byte_counts_the_reference_throws_on_are_refused(pkg, ctx, fmt, tail):
    """nbytes % elem != 0: status -3 from every entry-point family, host-fed and device-resident, and nothing is written."""
    n, W, lut = 64, 5, base._lut()
    win, bn = _taper(n)
    data = np.concatenate([tailref._signal(fmt, 4 * n, 0), tailref.TAIL_BYTES[:tail]])
    assert data.size % tailref.ELEM[fmt] != 0

    def refused(call):
        with pytest.raises(pkg.SpectroplotError) as e:
            call()
        assert e.value.status == -3, e.value

    refused(lambda: ctx.render(fmt, data, n, win, bn, GAIN, RANGE, lut, W))
    refused(lambda: ctx.render(fmt, data, n, win, bn, GAIN, RANGE, lut, W, detector="peak"))
    refused(lambda: ctx.render_batch(fmt, [data[:-tail], data], n, win, bn, GAIN, RANGE, lut, [W, W]))
    refused(lambda: ctx.render_index(fmt, data, n, win, bn, GAIN, RANGE, lut, W))
    refused(lambda: ctx.render_traces(fmt, data, n, win, bn, GAIN, RANGE, W))
    refused(lambda: ctx.render_power(fmt, data, n, win, bn, GAIN, RANGE, W))
    cap = _Capture(ctx, fmt, n, data)
    out = ss._Dev(ctx, 8 * W * n)
    ptrs, blk = base._alloc_reply(ctx, W, n, len(lut), False)
    iptrs, iblk = shapes._alloc(ctx, W, n, len(lut), 0)
    plans = [ctx.plan(fmt, n, win, bn, GAIN, RANGE, lut, detector=d) for d in ("sample", "peak")]
    try:
        for plan in plans:
            refused(lambda: plan.execute(cap.ptr, data.size, W, **ptrs))
        plan = plans[0]
        refused(lambda: plan.execute_batch([(cap.ptr, data.size - tail, W, ptrs), (cap.ptr, data.size, W, ptrs)]))
        refused(lambda: plan.execute_index(cap.ptr, data.size, W, **iptrs))
        refused(lambda: plan.execute_traces(cap.ptr, data.size, W, out.ptr, out.ptr + 8 * n))
        refused(lambda: plan.execute_power(cap.ptr, data.size, W, out.ptr))
        ctx.synchronize()
        assert (out.read(np.uint8, "refused") == 0xAB).all()
        assert (ctx.download(blk, 4 * W * n + 2 * base.GUARD) == 0xAB).all() and (ctx.download(iblk, W * n + 2 * base.GUARD) == 0xAB).all()
    finally:
        for plan in plans:
            plan.close()
        base._free_reply(ctx, ptrs, blk)
        shapes._free(ctx, iptrs, iblk)
        out.free()
        cap.free()
    RAN.add("refused_%s+%d" % (fmt, tail))


def test_zz_every_case_ran():
    """Runs last in the module: every case of the lattices, every batch and both refusals ran (and passed).  Prints the module's case
    count, total time and slowest case."""
    ids = IDS + BATCH_IDS + ["refused_%s+%d" % p for p in tailref.REFUSED]
    assert len(set(ids)) == len(ids) == 320 + 512 + 14 + 2
    assert RAN == set(ids), "%d of %d cases ran; missing %s" % (len(RAN), len(ids), sorted(set(ids) - RAN)[:8])
    slowest = max(TIMES, key=TIMES.get)
    print("\ntest_tails_gpu: %d cases, %.1f s in all, slowest %s %.2f s" % (len(TIMES), sum(TIMES.values()), slowest, TIMES[slowest]))
