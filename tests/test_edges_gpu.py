"""Every step of every output scale straddled on the GPU: the captures of tests/edgeref.py (|X|^2 a few ulps on either side of every
colour-index, centi-bel and gauge-byte edge; tests/test_edges_cpu.py shows with the oracle alone that they are what they claim)
through every frame-loop kernel and epilogue instantiation, compared with the C oracle.

Every comparison is exact and covers every reply field: rgba, gauge_mins, gauge_maxs, gauge_amps, c_hist, cB_hist and the bit patterns
of dBfs_min and dBfs_max.  Every case asserts which kernel served it, so a fall-back to the scratch kernel cannot make a case pass.
Tolerance: none."""
import numpy as np
import pytest

import edgeref
import peakref
from __graft_entry__ import load_package
from oracle import pyoracle

pytestmark = pytest.mark.gpu

FMT = edgeref.FMT
KERNEL_NAMES = {"frames": "frames", "scratch": "scratch_radix2"}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _bits(v):
    return int(np.float64(v).view(np.uint64))


def _frame_values(rgba, n, width, wf):
    """[frame, row, channel] of an image in either layout"""
    if wf:
        return rgba.reshape(width, n, 4)[::-1]
    return rgba.reshape(n, width, 4).transpose(1, 0, 2)


def _assert_same(got, want, what, n=None, width=None, wf=False, xs=None):
    """Every reply field, exactly; the first differing frames are named by edge, offset and x (hex) when the capture's x values are
    given, so that the f32 key the kernel formed can be recomputed from the plan's thresholds."""
    bad = []
    for k in ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps"):
        if not np.array_equal(got[k], want[k]):
            bad.append("%s differs in %d places" % (k, int(np.count_nonzero(got[k] != want[k]))))
    for k in ("c_hist", "cB_hist"):
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), want[k]):
            bad.append(k + " differs")
    for k in ("dBfs_min", "dBfs_max"):
        if _bits(got[k]) != _bits(want[k]):
            bad.append("%s %r (%016x), expected %r (%016x)" % (k, got[k], _bits(got[k]), want[k], _bits(want[k])))
    if bad and xs is not None and n is not None:
        frames = set()
        if got["rgba"].shape == want["rgba"].shape:
            frames |= set(np.nonzero((_frame_values(got["rgba"], n, width, wf) != _frame_values(want["rgba"], n, width, wf)).any(axis=(1, 2)))[0].tolist())
        for k in ("gauge_mins", "gauge_maxs", "gauge_amps"):
            frames |= set(np.nonzero(got[k] != want[k])[0].tolist())
        per = xs.shape[1] if xs.ndim == 2 else 1
        flat = xs.reshape(-1)
        for f in sorted(frames)[:8]:
            if f < flat.size:
                bad.append("frame %d: edge %d, offset index %d, x = %s, x*x = %s" % (f, f // per, f % per, float(flat[f]).hex(),
                                                                                      float(flat[f] * flat[f]).hex()))
    assert not bad, "%s: %s" % (what, "; ".join(bad))


class _Buffers:
    """The device outputs of one request shape, allocated once and reused across kernels."""
    KEYS = ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps", "c_hist", "cb_hist", "dbfs_minmax")

    def __init__(self, ctx, n, width, lut_len):
        self.ctx, self.n, self.width, self.lut_len = ctx, n, width, lut_len
        self.sizes = {"rgba": 4 * width * n, "gauge_mins": width, "gauge_maxs": width, "gauge_amps": width, "c_hist": 8 * lut_len,
                      "cb_hist": 8000, "dbfs_minmax": 16}
        self.ptrs = {k: ctx.alloc(max(v, 16)) for k, v in self.sizes.items()}

    def dirty(self):
        for k, v in self.sizes.items():
            self.ctx.memset(self.ptrs[k], 0xAB, max(v, 16))

    def read(self):
        c = self.ctx
        out = {k: c.download(self.ptrs[k], self.sizes[k]) for k in ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps")}
        out["c_hist"] = c.download(self.ptrs["c_hist"], 8 * self.lut_len, np.uint64)
        out["cB_hist"] = c.download(self.ptrs["cb_hist"], 8000, np.uint64)
        mm = c.download(self.ptrs["dbfs_minmax"], 16, np.float64)
        out["dBfs_min"], out["dBfs_max"] = float(mm[0]), float(mm[1])
        return out

    def free(self):
        for p in self.ptrs.values():
            self.ctx.free(p)


def _execute(ctx, plan, buf, d_in, nbytes):
    buf.dirty()
    plan.execute(d_in, nbytes, buf.width, **buf.ptrs)
    ctx.synchronize()
    return buf.read()


def _compare(pkg, ctx, ps, n, data, width, want, kernels, win, ch=False, wf=False, xs=None, detector="sample", auto=None):
    """The capture through each forced kernel of a plan for `ps`; one upload and one set of output buffers for all of them.
    kernels: {forced name: the kernel_name() it must report}; auto: what the plan must choose unforced."""
    plan = ctx.plan(FMT, n, win, ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), ch, wf, detector=detector)
    buf = _Buffers(ctx, n, width, ps.lut_len)
    d_in = ctx.alloc(data.size)
    try:
        if auto is not None:
            assert plan.kernel_name() == auto, (ps.name, plan.kernel_name())
        ctx.upload(d_in, data)
        for force, name in kernels.items():
            plan.force_kernel(force)
            served = plan.kernel_name(data.size, width)
            assert served == name, (ps.name, n, force, served)
            got = _execute(ctx, plan, buf, d_in, data.size)
            _assert_same(got, want, "%s n=%d %s%s [%s]" % (ps.name, n, "lr" if ch else "iq", " wf" if wf else "", served), n, width, wf, xs)
    finally:
        ctx.free(d_in)
        buf.free()
        plan.close()


# ---- a. the parameter sweep at n = 64 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ps", edgeref.SWEEP, ids=lambda p: p.name)
def test_sweep_of_the_accepted_domain_at_n64(pkg, ctx, ps):
    """All colour and centi-bel edges, offsets -2 .. +2, k_frames and the scratch kernel forced in turn, over the corners of
    plan_frames_capable's domain (edgeref.SWEEP says what each set strains).  Every set is one the plan gives to k_frames by itself.
    Reachability of the limits from request parameters: gray_b = 1.505 * lut_len / range reaches 2000 (the steep sets sit at 1541 and
    1927); g_m, c_m < 0.125 is not the binding limit anywhere inside gray_b <= 2000 and edges within 2^+-100 (the widest margin there
    is ~0.05 steps), so no accepted set comes near it; a gain in the hundreds is accepted only with a block_norm that brings the
    colour edges back inside 2^+-100, and its colour edges then lie outside the level scale's clamp range (gain outside [0, 100]),
    where every lane is decided against the exact tables."""
    n = 64
    e = edgeref.all_index_edges(ps)
    data, width, xs = edgeref.straddle_capture(e, n, edgeref.OFFSETS5)
    win = edgeref.taper(n, True)
    want = pyoracle.render(FMT, data, n, win, ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), width)
    _compare(pkg, ctx, ps, n, data, width, want, KERNEL_NAMES, win, xs=xs, auto="frames")


@pytest.mark.parametrize("ps", edgeref.OUTSIDE, ids=lambda p: p.name)
def test_sets_just_outside_the_domain_take_the_scratch_kernel(pkg, ctx, ps):
    n = 64
    e = edgeref.all_index_edges(ps)
    data, width, xs = edgeref.straddle_capture(e, n, edgeref.OFFSETS5)
    win = edgeref.taper(n, True)
    plan = ctx.plan(FMT, n, win, ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len))
    try:
        assert plan.kernel_name() == "scratch_radix2"
        with pytest.raises(pkg.SpectroplotError):
            plan.force_kernel("frames")
    finally:
        plan.close()
    want = pyoracle.render(FMT, data, n, win, ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), width)
    _compare(pkg, ctx, ps, n, data, width, want, {"auto": "scratch_radix2", "scratch": "scratch_radix2"}, win, xs=xs, auto="scratch_radix2")


# ---- b. every epilogue instantiation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", edgeref.EPILOGUE, ids=lambda c: "%s_n%d_%s%s" % (c[0].name, c[1], "lr" if c[2] else "iq", "_wf" if c[3] else ""))
def test_every_epilogue_instantiation(pkg, ctx, case):
    """n = 128 .. 8192 (byte tile, packed scales, late side outputs, frames shared by several waves), I/Q and L/R, both layouts per n;
    the default set under a flat taper and the most strained accepted set under a taper that is 1 only at index 0."""
    ps, n, ch, wf, flat, off = case
    data, width, xs = edgeref.straddle_capture(edgeref.all_index_edges(ps), n, off)
    win = edgeref.taper(n, flat)
    want = pyoracle.render(FMT, data, n, win, ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), width, ch, wf)
    _compare(pkg, ctx, ps, n, data, width, want, {"frames": "frames"}, win, ch, wf, xs=xs, auto="frames")


# ---- c. gauge edges and the device log10 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", edgeref.GAUGE_NS)
@pytest.mark.parametrize("ps", list(edgeref.GAUGE_SETS), ids=lambda p: p.name)
def test_gauge_byte_edges(pkg, ctx, ps, n):
    """gauge_mins / gauge_maxs (column extremes of the device log10) and gauge_amps (the raw centre sample) at every step of their
    byte: in-kernel side outputs of k_frames at n = 64, 1024, 2048 and, through the forced scratch kernel, k_finish_frames."""
    g = edgeref.gauge_edges(ps.gain, ps.rng, ps.block_norm)
    e0 = np.concatenate([g["mins"], g["maxs"]])
    d0, w0, x0 = edgeref.straddle_capture(e0, n, edgeref.OFFSETS5)
    d1, w1, x1 = edgeref.straddle_capture(g["amps"], n, edgeref.OFFSETS5, index=n // 2)
    data, width, xs = np.concatenate([d0, d1]), w0 + w1, np.concatenate([x0, x1])
    win = edgeref.taper(n, False)
    want = pyoracle.render(FMT, data, n, win, ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), width)
    assert len(np.unique(want["gauge_amps"])) == 256 and len(np.unique(want["gauge_mins"])) == 256
    _compare(pkg, ctx, ps, n, data, width, want, KERNEL_NAMES, win, xs=xs, auto="frames")


def _probe_frames(n):
    x = edgeref.log10_probe_values()
    frames = np.zeros((len(x), n, 2))
    frames[:, 0, 0] = x
    return x, [np.ascontiguousarray(f).reshape(-1).view(np.uint8) for f in frames]


def _probe_wants(n, datas, x):
    log10 = pyoracle.lib().spo_log10
    wants = []
    for d, v in zip(datas, x):
        want = pyoracle.render(FMT, d, n, edgeref.taper(n, True), 1.0, 0.0, 60.0, edgeref.lut(256), 1)
        # the exposure: the request's range IS the log10 result (block_norm = 1 and gain = 0 add exact zeros)
        d5 = 5 * log10(float(v) * float(v))
        assert (want["dBfs_min"], want["dBfs_max"]) == ((d5, -200.0) if d5 < -200 else (d5, d5) if d5 < 0 else (0.0, d5))
        wants.append(want)
    return wants


def test_device_log10_bit_for_bit_through_the_batch_kernel(pkg, ctx):
    """200 one-frame requests with block_norm = 1, gain = 0: dBfs_min / dBfs_max == 5 * log10(x*x), so every bit of the device's
    restated log10 is in the reply.  One batch of 200 items (k_frames_batch)."""
    n = 64
    x, datas = _probe_frames(n)
    wants = _probe_wants(n, datas, x)
    win = edgeref.taper(n, True)
    plan = ctx.plan(FMT, n, win, 1.0, 0.0, 60.0, edgeref.lut(256))
    assert plan.kernel_name() == "frames"
    plan.close()
    gf, grids, groups, rows = pkg.binding.debug_batch_plan(FMT, n, 256, 256, [d.size for d in datas], [1] * len(datas))
    assert gf >= 1 and all(r[0] in (0, 1) and r[2] == 1 for r in rows)
    outs = ctx.render_batch(FMT, datas, n, win, 1.0, 0.0, 60.0, edgeref.lut(256), [1] * len(datas))
    for k, (got, want) in enumerate(zip(outs, wants)):
        _assert_same(got, want, "item %d, x = %s" % (k, float(x[k]).hex()))


@pytest.mark.parametrize("n", edgeref.GAUGE_NS)
def test_device_log10_bit_for_bit_single_requests(pkg, ctx, n):
    """The same one-frame requests one by one through k_frames' side outputs (one shape per n) and the scratch kernel's k_finish_frames."""
    x, datas = _probe_frames(n)
    wants = _probe_wants(n, datas, x)
    win = edgeref.taper(n, True)
    plan = ctx.plan(FMT, n, win, 1.0, 0.0, 60.0, edgeref.lut(256))
    buf = _Buffers(ctx, n, 1, 256)
    d_in = ctx.alloc(datas[0].size)
    try:
        assert plan.kernel_name() == "frames"
        for force, name in KERNEL_NAMES.items():
            plan.force_kernel(force)
            assert plan.kernel_name(datas[0].size, 1) == name
            for k, (d, want) in enumerate(zip(datas, wants)):
                ctx.upload(d_in, d)
                _assert_same(_execute(ctx, plan, buf, d_in, d.size), want, "n=%d [%s] x = %s" % (n, name, float(x[k]).hex()))
    finally:
        ctx.free(d_in)
        buf.free()
        plan.close()


# ---- d. k_frames_batch ---------------------------------------------------------------------------------------------------------------

BATCH_WIDTHS = [1, 7, 33, 100, 257, 1000, 1500, 2000]          # ... and the rest of the capture as a ninth item


def _device_batch(ctx, plan, datas, widths, n, lut_len):
    bufs, ins, items = [], [], []
    for d, w in zip(datas, widths):
        b = _Buffers(ctx, n, w, lut_len)
        b.dirty()
        p = ctx.alloc(d.size)
        ctx.upload(p, d)
        bufs.append(b)
        ins.append(p)
        items.append((p, d.size, w, b.ptrs))
    try:
        plan.execute_batch(items)
        ctx.synchronize()
        return [b.read() for b in bufs]
    finally:
        for b in bufs:
            b.free()
        for p in ins:
            ctx.free(p)


@pytest.mark.parametrize("n", edgeref.BATCH_NS)
@pytest.mark.parametrize("ps", list(edgeref.BATCH_SETS), ids=lambda p: p.name)
def test_batch_kernel_at_every_edge(pkg, ctx, ps, n):
    """The straddle capture cut into nine items of unequal widths (one of width 1, odd ones that no group size divides) through
    sp_render_batch and sp_plan_execute_batch, each item against the oracle's render of its own bytes.  The library has no query for
    the kernel that served a batch: asserted are the plan's kernel, n inside k_frames_batch's domain (64 .. 512) and a work list with
    groups of the frame loop for every item (launch 0 or 1, never "one by one"); a kernel trace of this test shows k_frames_batch."""
    e = edgeref.all_index_edges(ps)
    data, width, xs = edgeref.straddle_capture(e, n, edgeref.OFFSETS5)
    widths = BATCH_WIDTHS + [width - sum(BATCH_WIDTHS)]
    assert len(widths) >= 8 and widths[-1] > 0 and 1 in widths
    fb = n * 16
    at = np.concatenate([[0], np.cumsum(widths)])
    datas = [data[at[k] * fb:at[k + 1] * fb] for k in range(len(widths))]
    win = edgeref.taper(n, ps is edgeref.DEFAULT)
    lut = edgeref.lut(ps.lut_len)
    wants = [pyoracle.render(FMT, d, n, win, ps.block_norm, ps.gain, ps.rng, lut, w) for d, w in zip(datas, widths)]
    assert 64 <= n <= 512
    gf, grids, groups, rows = pkg.binding.debug_batch_plan(FMT, n, ps.lut_len, 256, [d.size for d in datas], widths)
    assert gf >= 2 and any(w % gf for w in widths[1:])
    assert all(r[0] in (0, 1) and r[2] == -(-w // gf) for r, w in zip(rows, widths)), rows
    flat = xs.reshape(-1)
    plan = ctx.plan(FMT, n, win, ps.block_norm, ps.gain, ps.rng, lut)
    try:
        assert plan.kernel_name() == "frames"
        for how, outs in (("sp_render_batch", ctx.render_batch(FMT, datas, n, win, ps.block_norm, ps.gain, ps.rng, lut, widths)),
                          ("sp_plan_execute_batch", _device_batch(ctx, plan, datas, widths, n, ps.lut_len))):
            for k, (got, want) in enumerate(zip(outs, wants)):
                _assert_same(got, want, "%s n=%d %s item %d" % (ps.name, n, how, k), n, widths[k], False, flat[at[k]:at[k + 1]])
    finally:
        plan.close()


# ---- e. k_frames_peak ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", edgeref.PEAK_CASES, ids=lambda c: "%s_n%d_%s" % (c[0].name, c[1], "lr" if c[2] else "iq"))
def test_peak_kernel_holds_the_straddling_subframe(pkg, ctx, case):
    """M = 3 sub-frames per column; the straddling value in sub-frame 0, 1 or 2 beside silence, x / 2 or the double below x, the nine
    pairs rotating over the columns (edgeref.peak_capture), so the held maximum decides the side of the edge.  k_frames_peak (the L/R variants at n >= 256 reload
    spilled registers in the sub-frame loop) and the scratch kernel against tests/peakref.py's fold of the oracle's planes."""
    ps, n, ch = case
    data, width, col_x, _ = edgeref.peak_capture(edgeref.peak_edge_subset(ps, n), n, edgeref.OFFSETS5)
    win = edgeref.taper(n, ps is edgeref.DEFAULT)
    want = peakref.expected(FMT, data, n, win, ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), width, ch, False)
    assert want["M"] == edgeref.PEAK_M and want["counts"][:-1] == [edgeref.PEAK_M] * (width - 1)
    assert pkg.binding.peak_subframes(FMT, n, data.size, width) == (edgeref.PEAK_M, 1)
    _compare(pkg, ctx, ps, n, data, width, want, {"frames": "frames_peak", "scratch": "scratch_radix2"}, win, ch, False, xs=col_x,
             detector="peak")
