"""The exact mean-power trace on the GPU (sp_power_mean, sp_plan_execute_mean, sp_render_mean): every comparison is bit for bit
against tests/meanref.py - math.fsum per column divided by the width - on the oracle's plane (tests/powerref.py) or on a synthetic one
(which NaN a NaN is, is the one thing left uncompared).  Every device result lies between guard bytes and holds garbage before the call.

The measurement that goes with the feature is not asserted here (tools/mean_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import meanref
import powerref
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle
from test_gpu_parity import _assert_same as assert_same_reply

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 31415, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
GARBAGE = 0xAB
GUARD = 4096
WIDTHS = [1, 2, 37, 300]
FORMATS = ["CU8", "CS16", "CF32"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Out:
    """A device array f64[n] between two guards, everything garbage."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.base = ctx.alloc(8 * n + 2 * GUARD)
        assert self.base % 8 == 0
        self.ptr = self.base + GUARD
        ctx.memset(self.base, GARBAGE, 8 * n + 2 * GUARD)

    def read(self, what=""):
        whole = self.ctx.download(self.base, 8 * self.n + 2 * GUARD)
        assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + 8 * self.n:] == GARBAGE).all(), what + ": bytes around the mean were written"
        return whole[GUARD:GUARD + 8 * self.n].view(np.float64).copy()

    def free(self):
        self.ctx.free(self.base)


def _upload(ctx, data):
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    d = ctx.alloc(max(data.size, 16))
    if data.size:
        ctx.upload(d, data)
    return d


def _capture(fmt, n, width, stride_num, stride_den=1, extra=0):
    samples = n + (max(width, 1) - 1) * stride_num // stride_den + extra
    return siggen.generate(fmt, GEN, samples)


def _power_mean(ctx, plane, what):
    """sp_power_mean of a host plane f64 [width, n] through a device copy."""
    width, n = plane.shape
    d_p, out = _upload(ctx, plane), _Out(ctx, n)
    try:
        ctx.power_mean(d_p if width else 0, n, width, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_p)
        out.free()


def _execute_mean(ctx, plan, d_in, nbytes, width, n, what):
    out = _Out(ctx, n)
    try:
        plan.execute_mean(d_in, nbytes, width, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


# ---- (a) sp_power_mean on synthetic planes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(n, width):
    plane = meanref.synthetic_plane(1000 * n + width, width, n)
    plane.setflags(write=False)
    want = meanref.expected(plane)
    want.setflags(write=False)
    return plane, want


@pytest.mark.parametrize("width", [1, 2, 3, 257, 1025])
@pytest.mark.parametrize("n", [2, 32, 64, 100, 256])
def test_power_mean_of_synthetic_planes(ctx, n, width):
    """The full exponent range, denormals, cell-boundary exponents, ties at 2^53 and sums past DBL_MAX; n = 100 is no multiple of the
    kernel's band of rows, widths 257 and 1025 give the workgroups ragged pieces of the frames."""
    plane, want = _synthetic(n, width)
    if n >= 6 and width >= 2:
        assert np.isinf(want[5]) and want[2] < 2.0 ** -1022
    meanref.assert_same(_power_mean(ctx, plane, "n=%d W=%d" % (n, width)), want, "sp_power_mean n=%d W=%d" % (n, width))


def test_power_mean_nan_and_inf_rule(ctx):
    n, width = 64, 257
    plane = _synthetic(n, width)[0].copy()
    plane[100, 7] = np.nan            # a NaN in one frame of one row
    plane[3, 12] = np.inf             # an inf in another
    plane[200, 13] = np.inf
    plane[201, 13] = np.nan           # NaN beats inf
    plane[5, 5] = np.inf              # (that row overflows anyway)
    want = meanref.expected(plane)
    assert np.isnan(want[7]) and want[12] == np.inf and np.isnan(want[13]) and np.isfinite(want[6])
    meanref.assert_same(_power_mean(ctx, plane, "specials"), want, "sp_power_mean specials")


@pytest.mark.parametrize("n", [2, 64, 256])
def test_power_mean_of_no_frames_is_nan(ctx, n):
    got = _power_mean(ctx, np.zeros((0, n)), "width 0")
    assert np.isnan(got).all()


# ---- (b) sp_plan_execute_mean against the oracle's plane --------------------------------------------------------------------------------------
# (n, forced onto the portable kernel, the frame loop's name)
KERNELS = [(64, False, "frames_power"), (256, False, "frames_power"), (1024, False, "frames_power"),
           (32, False, "scratch_power"), (2048, False, "scratch_power"), (256, True, "scratch_power")]


@functools.lru_cache(maxsize=None)
def _reference(fmt, n, width, ch, stride):
    data = _capture(fmt, n, width, stride)
    win, weight = pyoracle.window("hann", n)
    want = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, ch)
    powerref.assert_telling(want["power"][:, 1:] if ch else want["power"], "%s n=%d W=%d" % (fmt, n, width))
    mean = meanref.expected(want["power"])
    for a in (data, win, want["power"], mean):
        a.setflags(write=False)
    return data, win, 1.0 / weight, want["power"], mean


@pytest.mark.parametrize("k", range(len(KERNELS)), ids=["n%d%s" % (n, "-forced" if f else "") for n, f, _ in KERNELS])
@pytest.mark.parametrize("j", range(len(WIDTHS)), ids=["W%d" % w for w in WIDTHS])
def test_execute_mean_against_the_oracle(ctx, k, j):
    """Every (kernel, n) at every width; the format and the channel mode rotate so that each format and both modes meet each kernel."""
    n, forced, name = KERNELS[k]
    width = WIDTHS[j]
    fmt, ch = FORMATS[(k + j) % 3], (k // 3 + j) % 2 == 1
    data, win, bn, _, want = _reference(fmt, n, width, ch, n // 2 + 3)
    what = "%s n=%d W=%d%s%s" % (fmt, n, width, " L/R" if ch else "", " forced" if forced else "")
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.mean_kernel_name_for(data.size, width) == name + "+mean"
        meanref.assert_same(_execute_mean(ctx, plan, d_in, data.size, width, n, what), want, what)
    finally:
        ctx.free(d_in)
        plan.close()
    if ch:
        assert want.view(np.uint64)[0] == 0          # the split's row 0 is +0.0 in every frame


def test_every_format_meets_both_channel_modes_and_kernels():
    seen = set()
    for k, (n, forced, name) in enumerate(KERNELS):
        for j in range(len(WIDTHS)):
            seen.add((FORMATS[(k + j) % 3], (k // 3 + j) % 2 == 1, name))
    assert len(seen) == 3 * 2 * 2


# ---- (c) order-freedom ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 256, 300, False), ("CF32", 1024, 37, True), ("CU8", 2048, 37, False)])
def test_the_window_does_not_change_a_bit(ctx, fmt, n, width, ch):
    data, win, bn, _, want = _reference(fmt, n, width, ch, n // 2 + 3)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    got = []
    try:
        for window in (8 * n, 3 * 8 * n, 0):
            ctx.set_mean_window(window)
            got.append(_execute_mean(ctx, plan, d_in, data.size, width, n, "window %d" % window))
        ctx.set_mean_window(1)                       # below one frame: one frame
        got.append(_execute_mean(ctx, plan, d_in, data.size, width, n, "window 1"))
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()
    for g in got:
        meanref.assert_same(g, want, "window")
        assert np.array_equal(g.view(np.uint64), got[0].view(np.uint64))


# ---- (d) consistency with what exists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 256, 300, False), ("CF32", 1024, 37, True), ("CU8", 2048, 37, False)])
def test_mean_lies_between_the_traces_and_is_the_mean_of_the_plane(ctx, fmt, n, width, ch):
    data, win, bn, _, want = _reference(fmt, n, width, ch, n // 2 + 3)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    d_tr, d_plane = ctx.alloc(16 * n), ctx.alloc(8 * width * n)
    mean, db, from_plane = _Out(ctx, n), _Out(ctx, n), _Out(ctx, n)
    try:
        plan.execute_mean(d_in, data.size, width, mean.ptr)
        plan.power_to_db(mean.ptr, n, db.ptr)
        plan.execute_traces(d_in, data.size, width, d_tr, d_tr + 8 * n)
        plan.execute_power(d_in, data.size, width, d_plane)
        ctx.power_mean(d_plane, n, width, from_plane.ptr)
        ctx.synchronize()
        tr = ctx.download(d_tr, 16 * n, np.float64)
        got, got_db, got_plane = mean.read("mean"), db.read("dB"), from_plane.read("from the plane")
    finally:
        for p in (d_in, d_tr, d_plane):
            ctx.free(p)
        for o in (mean, db, from_plane):
            o.free()
        plan.close()
    meanref.assert_same(got, want, "sp_plan_execute_mean")
    assert np.array_equal(got.view(np.uint64), got_plane.view(np.uint64))
    assert not np.isnan(got_db).any()
    assert (tr[:n] <= got_db).all() and (got_db <= tr[n:]).all()
    if not ch:
        assert (tr[:n] < tr[n:]).all()               # a request whose traces leave room to be wrong in


# ---- (e) the host entry point -------------------------------------------------------------------------------------------------------------------
def test_small_sparse_request_uploads_its_frames_only(ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, want = _reference(fmt, n, width, False, 40 * n + 11)
    got = ctx.render_mean(fmt, data, n, win, bn, 3.0, 50.0, width, fill=GARBAGE)
    meanref.assert_same(got, want, "sparse sp_render_mean")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1


def test_db_form_is_power_to_db_of_the_mean(ctx):
    fmt, n, width = "CS16", 256, 300
    data, win, bn, _, want = _reference(fmt, n, width, False, n // 2 + 3)
    got = ctx.render_mean(fmt, data, n, win, bn, 3.0, 50.0, width, fill=GARBAGE)
    got_db = ctx.render_mean(fmt, data, n, win, bn, 3.0, 50.0, width, db=True, fill=GARBAGE)
    meanref.assert_same(got, want, "sp_render_mean")
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_m, out = _upload(ctx, got), _Out(ctx, n)
    try:
        plan.power_to_db(d_m, n, out.ptr)
        ctx.synchronize()
        want_db = out.read("dB")
    finally:
        ctx.free(d_m)
        out.free()
        plan.close()
    assert np.isfinite(want_db).all() and len(np.unique(want_db)) > n // 2
    assert np.array_equal(got_db.view(np.uint64), want_db.view(np.uint64))
    meanref.assert_same(got_db, meanref.db_of(want, bn, 3.0), "sp_render_mean db against the oracle's log10")


@pytest.mark.parametrize("fmt,n,width,name", [("CF32", 2048, 1024, "scratch_power+mean"), ("CF32", 1024, 2048, "frames_power+mean")])
def test_chunked_sp_render_mean(ctx, fmt, n, width, name):
    """stride n, 16 MiB - the smallest request the streamer cuts (the first shape is the traces' chunked test on the portable kernel; the
    second takes the frame loop): the capture travels in chunks and the cells accumulate over them."""
    data, win, bn, _, want = _reference(fmt, n, width, False, n)
    assert data.size >= 16 << 20
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    try:
        assert plan.mean_kernel_name_for(data.size, width) == name
    finally:
        plan.close()
    got = ctx.render_mean(fmt, data, n, win, bn, 3.0, 50.0, width, fill=GARBAGE)
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    meanref.assert_same(got, want, "chunked sp_render_mean")


@pytest.mark.parametrize("n", [64, 2048])
def test_capture_shorter_than_n_gives_nan_everywhere(ctx, n):
    data = siggen.generate("CS16", GEN, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    got = ctx.render_mean("CS16", data, n, win, 1.0 / weight, 3.0, 50.0, 3, fill=0)
    assert np.isnan(got).all()
    got = ctx.render_mean("CS16", data, n, win, 1.0 / weight, 3.0, 50.0, 0, fill=0)          # ... and so does a request of no frames
    assert np.isnan(got).all()


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    d_in, d_out, d_plane = ctx.alloc(data.size), ctx.alloc(8 * n + 16), ctx.alloc(8 * width * n + 16)
    vp = C.c_void_p
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_mean(d_in, data.size, width, d_out)
        assert e.value.status == -4 and "peak" in str(e.value)
        assert L.sp_plan_execute_mean(None, vp(d_in), data.size, width, vp(d_out)) == -1
        assert L.sp_plan_execute_mean(plan.h, vp(d_in), data.size, width, vp(d_out + 4)) == -1      # misaligned
        assert L.sp_plan_execute_mean(plan.h, vp(d_in), data.size, width, None) == -1               # NULL
        assert L.sp_plan_execute_mean(plan.h, vp(d_in), data.size, 0, None) == -1                   # ... at width 0 too: n NaNs are written
        assert L.sp_plan_execute_mean(plan.h, vp(d_in), data.size, -1, vp(d_out)) == -1
        assert L.sp_plan_execute_mean(plan.h, None, data.size, width, vp(d_out)) == -1
        plan16 = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
        assert L.sp_plan_execute_mean(plan16.h, vp(d_in), 4 * 100 + 1, width, vp(d_out)) == -3
        plan16.close()
        assert L.sp_power_mean(None, vp(d_plane), n, width, vp(d_out)) == -1
        assert L.sp_power_mean(ctx.h, vp(d_plane), 0, width, vp(d_out)) == -1
        assert L.sp_power_mean(ctx.h, vp(d_plane), n, -1, vp(d_out)) == -1
        assert L.sp_power_mean(ctx.h, vp(d_plane + 4), n, width, vp(d_out)) == -1
        assert L.sp_power_mean(ctx.h, vp(d_plane), n, width, vp(d_out + 2)) == -1
        assert L.sp_power_mean(ctx.h, vp(d_plane), n, width, None) == -1
        assert L.sp_power_mean(ctx.h, None, n, width, vp(d_out)) == -1
        assert L.sp_plan_mean_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
    finally:
        peak.close()
        plan.close()
        for p_ in (d_in, d_out, d_plane):
            ctx.free(p_)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "peak")
    out = np.zeros(n)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    assert L.sp_render_mean(ctx.h, C.byref(req), p(data), data.size, width, 0, p(out)) == -4
    req.detector = 0
    assert L.sp_render_mean(None, C.byref(req), p(data), data.size, width, 0, p(out)) == -1
    assert L.sp_render_mean(ctx.h, None, p(data), data.size, width, 0, p(out)) == -1
    assert L.sp_render_mean(ctx.h, C.byref(req), None, data.size, width, 0, p(out)) == -1
    assert L.sp_render_mean(ctx.h, C.byref(req), p(data), data.size, -2, 0, p(out)) == -1
    assert L.sp_render_mean(ctx.h, C.byref(req), p(data), data.size, width, 0, None) == -1
    assert L.sp_render_mean(ctx.h, C.byref(req), p(data), data.size, width, 0, vp(out.ctypes.data + 4)) == -1
    assert L.sp_render_mean(ctx.h, C.byref(req), p(data), data.size, width, 0, p(out)) == 0
    assert np.isfinite(out).all() and (out > 0).all()


# ---- (g) interleaving -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width", [("CS16", 256, 300), ("CU8", 2048, 37)])
def test_execute_and_execute_mean_interleave_without_a_synchronisation(ctx, fmt, n, width):
    data, win, bn, _, want = _reference(fmt, n, width, False, n // 2 + 3)
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    r_want = pyoracle.render(fmt, data, n, win, bn, 3.0, 50.0, lut, width)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, lut)
    d_in = _upload(ctx, data)
    sizes = [4 * width * n, width, width, width, 8 * 256, 8000, 16]
    first = [ctx.alloc(s_) for s_ in sizes]
    second = [ctx.alloc(s_) for s_ in sizes]
    out = _Out(ctx, n)

    def reply(ptrs):
        got = {"rgba": ctx.download(ptrs[0], sizes[0]), "gauge_mins": ctx.download(ptrs[1], width), "gauge_maxs": ctx.download(ptrs[2], width),
               "gauge_amps": ctx.download(ptrs[3], width), "c_hist": ctx.download(ptrs[4], 8 * 256, np.uint64),
               "cB_hist": ctx.download(ptrs[5], 8000, np.uint64)}
        mm = ctx.download(ptrs[6], 16, np.float64)
        got["dBfs_min"], got["dBfs_max"] = float(mm[0]), float(mm[1])
        return got

    try:
        for p_, s_ in zip(first + second, sizes + sizes):
            ctx.memset(p_, 0xA5, s_)
        ctx.synchronize()
        plan.execute(d_in, data.size, width, *first)
        plan.execute_mean(d_in, data.size, width, out.ptr)
        plan.execute(d_in, data.size, width, *second)
        ctx.synchronize()
        assert_same_reply(reply(first), r_want)
        assert_same_reply(reply(second), r_want)
        meanref.assert_same(out.read("interleaved"), want, "interleaved")
    finally:
        out.free()
        for p_ in first + second + [d_in]:
            ctx.free(p_)
        plan.close()
