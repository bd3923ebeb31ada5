"""The exact band-power series on the GPU (sp_power_bands, sp_plan_execute_bandpower, sp_render_bandpower): every comparison is bit for
bit against tests/bandref.py - math.fsum over a band's rows of every frame - on the oracle's plane (tests/powerref.py, the references
of tests/test_mean_gpu.py shared) or on a synthetic one (which NaN a NaN is, is the one thing left uncompared).  Every result lies
between guard bytes and holds garbage before the call.

The measurement that goes with the feature is not asserted here (tools/band_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bandref
import meanref
import powerref
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle
from test_gpu_parity import _assert_same as assert_same_reply
from test_mean_gpu import FORMATS, GARBAGE, GEN, GUARD, KERNELS, WIDTHS, _capture, _reference, _upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Out:
    """A device array f64 [count, width] between two guards, everything garbage."""

    def __init__(self, ctx, count, width):
        self.ctx, self.shape, self.bytes = ctx, (count, width), 8 * count * width
        self.base = ctx.alloc(self.bytes + 2 * GUARD)
        assert self.base % 8 == 0
        self.ptr = self.base + GUARD
        ctx.memset(self.base, GARBAGE, self.bytes + 2 * GUARD)

    def whole(self):
        return self.ctx.download(self.base, self.bytes + 2 * GUARD)

    def read(self, what=""):
        whole = self.whole()
        assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + self.bytes:] == GARBAGE).all(), what + ": bytes around the series were written"
        return whole[GUARD:GUARD + self.bytes].view(np.float64).reshape(self.shape).copy()

    def free(self):
        self.ctx.free(self.base)


def _power_bands(ctx, plane, bands, what):
    """sp_power_bands of a host plane f64 [width, n] through a device copy."""
    width, n = plane.shape
    d_p, out = _upload(ctx, plane), _Out(ctx, len(bands), width)
    try:
        ctx.power_bands(d_p if width else 0, n, width, bands, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_p)
        out.free()


def _execute_bandpower(ctx, plan, d_in, nbytes, width, bands, what):
    out = _Out(ctx, len(bands), width)
    try:
        plan.execute_bandpower(d_in, nbytes, width, bands, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


@functools.lru_cache(maxsize=None)
def _want(fmt, n, width, ch, stride):
    """The series of bandref.standard_bands(n) over the plane test_mean_gpu's reference holds for this request."""
    plane = _reference(fmt, n, width, ch, stride)[3]
    want = bandref.expected(plane, bandref.standard_bands(n))
    want.setflags(write=False)
    return want


# ---- (a) sp_power_bands on synthetic planes ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(n, width):
    plane = bandref.synthetic_plane(7000 * n + width, n, width)
    plane.setflags(write=False)
    want = bandref.expected(plane, bandref.standard_bands(n))
    want.setflags(write=False)
    return plane, want


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("n", [2, 64, 100, 256])
def test_power_bands_of_synthetic_planes(ctx, n, width):
    """Frames over the full exponent range (64 values of a load in up to 64 different cells), denormals, cell-boundary exponents, ties
    at 2^53 and a frame whose sum passes DBL_MAX; n = 100 is no multiple of a load's 64 rows, widths 1 and 2 are less than a
    workgroup's frames, 63, 65 and 257 no multiple of them, 64 is one."""
    plane, want = _synthetic(n, width)
    bands = bandref.standard_bands(n)
    if width > 5 and n >= 4:
        assert np.isinf(want[2, 5]) and 0 < want[2, 2] < 2.0 ** -1022 * n
    got = _power_bands(ctx, plane, bands, "n=%d W=%d" % (n, width))
    bandref.assert_same(got, want, "sp_power_bands n=%d W=%d" % (n, width))
    assert (got[0].view(np.uint64) == 0).all()                                               # the empty band: +0.0
    assert np.array_equal(got[1].view(np.uint64), plane[:, 0].copy().view(np.uint64))          # one row: the plane's column, bit for bit
    assert np.array_equal(got[5].view(np.uint64), plane[:, n - 1].copy().view(np.uint64))


def test_power_bands_with_the_most_bands(ctx):
    n, width = 100, 65
    plane = _synthetic(n, width)[0]
    bands = [(k, min(n, k + k % 7)) for k in range(bandref.SP_MAX_BANDS)]
    assert len(bands) == 64 and any(y0 == y1 for y0, y1 in bands)
    bandref.assert_same(_power_bands(ctx, plane, bands, "64 bands"), bandref.expected(plane, bands), "sp_power_bands with 64 bands")


def test_power_bands_nan_and_inf_rule(ctx):
    n, width = 100, 65
    plane = _synthetic(n, width)[0].copy()
    plane[7, 10] = np.nan             # a NaN in one row of one frame
    plane[12, 3] = np.inf             # an inf in another
    plane[13, 70] = np.inf
    plane[13, 71] = np.nan            # NaN beats inf
    plane[5, 5] = np.inf              # (that frame overflows anyway)
    plane[64, 99] = np.nan            # the last frame's last row
    bands = bandref.standard_bands(n) + [(10, 11), (11, 71), (70, 72), (71, 100)]
    want = bandref.expected(plane, bands)
    assert np.isnan(want[2, 7]) and want[2, 12] == np.inf and np.isnan(want[2, 13]) and np.isfinite(want[2, 6])
    assert np.isnan(want[8, 7]) and np.isfinite(want[9, 7]) and want[9, 13] == np.inf and np.isnan(want[10, 13]) and np.isnan(want[11, 64])
    bandref.assert_same(_power_bands(ctx, plane, bands, "specials"), want, "sp_power_bands specials")


# ---- (b) sp_plan_execute_bandpower against the oracle's plane --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(KERNELS)), ids=["n%d%s" % (n, "-forced" if f else "") for n, f, _ in KERNELS])
@pytest.mark.parametrize("j", range(len(WIDTHS)), ids=["W%d" % w for w in WIDTHS])
def test_execute_bandpower_against_the_oracle(ctx, k, j):
    """Every (kernel, n) at every width; the format and the channel mode rotate as in test_mean_gpu.py, so that each format and both
    modes meet each kernel."""
    n, forced, name = KERNELS[k]
    width = WIDTHS[j]
    fmt, ch = FORMATS[(k + j) % 3], (k // 3 + j) % 2 == 1
    data, win, bn, plane, _ = _reference(fmt, n, width, ch, n // 2 + 3)
    want = _want(fmt, n, width, ch, n // 2 + 3)
    what = "%s n=%d W=%d%s%s" % (fmt, n, width, " L/R" if ch else "", " forced" if forced else "")
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.bandpower_kernel_name_for(data.size, width) == name + "+bands"
        got = _execute_bandpower(ctx, plan, d_in, data.size, width, bandref.standard_bands(n), what)
    finally:
        ctx.free(d_in)
        plan.close()
    bandref.assert_same(got, want, what)
    assert np.array_equal(got[5].view(np.uint64), plane[:, n - 1].copy().view(np.uint64))
    assert (got[2] >= got[6]).all() and (got[2] >= got[7]).all() and (got[2] > 0).all()      # the whole spectrum holds its parts


# ---- (c) order-freedom ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 256, 300, False), ("CF32", 1024, 37, True), ("CU8", 2048, 37, False)])
def test_the_window_does_not_change_a_bit(ctx, fmt, n, width, ch):
    data, win, bn, _, _ = _reference(fmt, n, width, ch, n // 2 + 3)
    want, bands = _want(fmt, n, width, ch, n // 2 + 3), bandref.standard_bands(n)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    got = []
    try:
        for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, below one frame (one frame), the default
            ctx.set_mean_window(window)
            got.append(_execute_bandpower(ctx, plan, d_in, data.size, width, bands, "window %d" % window))
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()
    for g in got:
        bandref.assert_same(g, want, "window")
        assert np.array_equal(g.view(np.uint64), got[0].view(np.uint64))


# ---- (d) consistency with what exists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 256, 300, False), ("CF32", 1024, 37, True), ("CU8", 2048, 37, False)])
def test_bands_of_the_plane_are_the_bands_of_the_request_and_the_db_form(ctx, fmt, n, width, ch):
    data, win, bn, _, _ = _reference(fmt, n, width, ch, n // 2 + 3)
    want, bands = _want(fmt, n, width, ch, n // 2 + 3), bandref.standard_bands(n)
    count = len(bands)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in, d_plane = _upload(ctx, data), ctx.alloc(8 * width * n)
    direct, db, from_plane = _Out(ctx, count, width), _Out(ctx, count, width), _Out(ctx, count, width)
    try:
        plan.execute_bandpower(d_in, data.size, width, bands, direct.ptr)
        plan.power_to_db(direct.ptr, count * width, db.ptr)
        plan.execute_power(d_in, data.size, width, d_plane)
        ctx.power_bands(d_plane, n, width, bands, from_plane.ptr)
        ctx.synchronize()
        got, got_db, got_plane = direct.read("direct"), db.read("dB"), from_plane.read("from the plane")
    finally:
        for p in (d_in, d_plane):
            ctx.free(p)
        for o in (direct, db, from_plane):
            o.free()
        plan.close()
    bandref.assert_same(got, want, "sp_plan_execute_bandpower")
    assert np.array_equal(got.view(np.uint64), got_plane.view(np.uint64))
    want_db = meanref.db_of(want.reshape(-1), bn, 3.0).reshape(want.shape)
    bandref.assert_same(got_db, want_db, "sp_plan_power_to_db of the sums against the oracle's log10")
    assert np.isneginf(got_db[0]).all() and np.isfinite(got_db[2]).all()
    # ... and the host entry's dB form is the same conversion
    host_db = ctx.render_bandpower(fmt, data, n, win, bn, 3.0, 50.0, width, bands, ch, db=True, fill=GARBAGE)
    assert np.array_equal(host_db.view(np.uint64), got_db.view(np.uint64))


# ---- (e) the host entry point -------------------------------------------------------------------------------------------------------------------
def _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands, ch=False, db=0):
    """sp_render_bandpower into a host array between guards, everything garbage: (status, the series, the guards are intact)."""
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, ch, False)
    b = np.ascontiguousarray(np.asarray(bands, np.int32).reshape(-1, 2))
    count, size = b.shape[0], 8 * b.shape[0] * max(width, 0)
    host = np.full(size + 2 * GUARD, GARBAGE, np.uint8)
    out = host[GUARD:GUARD + size]
    vp = C.c_void_p
    rc = ctx.lib.L.sp_render_bandpower(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, width, b.ctypes.data_as(vp) if count else None,
                                       count, db, vp(host.ctypes.data + GUARD))
    intact = bool((host[:GUARD] == GARBAGE).all() and (host[GUARD + size:] == GARBAGE).all())
    return rc, out.view(np.float64).reshape(count, max(width, 0)).copy(), intact


def test_small_sparse_request_uploads_its_frames_only(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, _ = _reference(fmt, n, width, False, 40 * n + 11)
    want, bands = _want(fmt, n, width, False, 40 * n + 11), bandref.standard_bands(n)
    rc, got, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands)
    assert rc == 0 and intact
    bandref.assert_same(got, want, "sparse sp_render_bandpower")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1
    bandref.assert_same(ctx.render_bandpower(fmt, data, n, win, bn, 3.0, 50.0, width, bands, fill=GARBAGE), want, "Context.render_bandpower")


def test_chunked_sp_render_bandpower(pkg, ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts: the capture travels in chunks and every chunk fills its columns."""
    fmt, n, width = "CF32", 1024, 2048
    data, win, bn, _, _ = _reference(fmt, n, width, False, n)
    want, bands = _want(fmt, n, width, False, n), bandref.standard_bands(n)
    assert data.size >= 16 << 20
    rc, got, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands)
    assert rc == 0 and intact
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    bandref.assert_same(got, want, "chunked sp_render_bandpower")


@pytest.mark.parametrize("n", [64, 2048])
def test_capture_shorter_than_n_gives_nan_everywhere(pkg, ctx, n):
    data = siggen.generate("CS16", GEN, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    rc, got, intact = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, 3, [(0, n), (1, 2), (n - 1, n)])
    assert rc == 0 and intact and got.shape == (3, 3) and np.isnan(got).all()
    rc, got, intact = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, 3, [(0, n), (5, 5)])
    assert rc == 0 and intact and np.isnan(got[0]).all() and (got[1].view(np.uint64) == 0).all()      # an empty band has no NaN addend


def test_width_0_and_count_0_write_nothing(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, _ = _reference(fmt, n, width, False, 40 * n + 11)
    vp = C.c_void_p
    # the host entry: its `band` lies inside a garbage array, of which nothing may change
    for w, bands in ((0, [(0, n), (3, 9)]), (width, [])):
        req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, False, False)
        b = np.asarray(bands, np.int32).reshape(-1, 2)
        host = np.full(2 * GUARD, GARBAGE, np.uint8)
        for out in (vp(host.ctypes.data + GUARD), None):
            assert ctx.lib.L.sp_render_bandpower(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, w,
                                                 b.ctypes.data_as(vp) if len(bands) else None, len(bands), 0, out) == 0
        assert (host == GARBAGE).all()
    # the device entries
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in, d_plane, out = _upload(ctx, data), ctx.alloc(8 * width * n), _Out(ctx, 1, 1)
    try:
        plan.execute_bandpower(d_in, data.size, 0, [(0, n)], out.ptr)
        plan.execute_bandpower(d_in, data.size, width, [], out.ptr)
        plan.execute_bandpower(d_in, data.size, 0, [(0, n)], 0)
        plan.execute_bandpower(d_in, data.size, width, [], 0)
        ctx.power_bands(d_plane, n, 0, [(0, n)], out.ptr)
        ctx.power_bands(d_plane, n, width, [], out.ptr)
        ctx.power_bands(0, n, 0, [(0, n)], 0)
        ctx.synchronize()
        assert (out.whole() == GARBAGE).all()
    finally:
        out.free()
        for p in (d_in, d_plane):
            ctx.free(p)
        plan.close()


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    d_in, d_out, d_plane = ctx.alloc(data.size), ctx.alloc(8 * 64 * width + 16), ctx.alloc(8 * width * n + 16)
    vp = C.c_void_p

    def arr(*rows):
        return (C.c_int32 * len(rows))(*rows)

    ok, many = arr(0, n, 3, 9), arr(*([0, 1] * 65))
    bad_bands = [(arr(0, n + 1), 1), (arr(-1, 4), 1), (arr(5, 4), 1), (arr(0, n, n + 1, n + 1), 2), (many, 65), (ok, -1), (None, 1)]
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_bandpower(d_in, data.size, width, [(0, n)], d_out)
        assert e.value.status == -4 and "peak" in str(e.value)
        ex = L.sp_plan_execute_bandpower
        assert ex(None, vp(d_in), data.size, width, ok, 2, vp(d_out)) == -1
        for bands, count in bad_bands:
            assert ex(plan.h, vp(d_in), data.size, width, bands, count, vp(d_out)) == -1, count
            assert L.sp_power_bands(ctx.h, vp(d_plane), n, width, bands, count, vp(d_out)) == -1, count
        assert ex(plan.h, vp(d_in), data.size, width, many, 64, vp(d_out)) == 0                 # 64 bands are allowed
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, vp(d_out + 4)) == -1               # misaligned
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, None) == -1                        # NULL
        assert ex(plan.h, vp(d_in), data.size, -1, ok, 2, vp(d_out)) == -1
        assert ex(plan.h, None, data.size, width, ok, 2, vp(d_out)) == -1
        plan16 = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
        assert ex(plan16.h, vp(d_in), 4 * 100 + 1, width, ok, 2, vp(d_out)) == -3
        plan16.close()
        pb = L.sp_power_bands
        assert pb(None, vp(d_plane), n, width, ok, 2, vp(d_out)) == -1
        assert pb(ctx.h, vp(d_plane), 0, width, arr(0, 0), 1, vp(d_out)) == -1
        assert pb(ctx.h, vp(d_plane), n, -1, ok, 2, vp(d_out)) == -1
        assert pb(ctx.h, vp(d_plane + 4), n, width, ok, 2, vp(d_out)) == -1
        assert pb(ctx.h, vp(d_plane), n, width, ok, 2, vp(d_out + 2)) == -1
        assert pb(ctx.h, vp(d_plane), n, width, ok, 2, None) == -1
        assert pb(ctx.h, None, n, width, ok, 2, vp(d_out)) == -1
        assert pb(ctx.h, vp(d_plane), 100, width, arr(0, 101), 1, vp(d_out)) == -1               # any n >= 1: its own bound
        assert L.sp_plan_bandpower_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
    finally:
        peak.close()
        plan.close()
        for p_ in (d_in, d_out, d_plane):
            ctx.free(p_)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "peak")
    out = np.zeros(64 * width)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    rb = L.sp_render_bandpower
    assert rb(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, p(out)) == -4
    req.detector = 0
    assert rb(None, C.byref(req), p(data), data.size, width, ok, 2, 0, p(out)) == -1
    assert rb(ctx.h, None, p(data), data.size, width, ok, 2, 0, p(out)) == -1
    assert rb(ctx.h, C.byref(req), None, data.size, width, ok, 2, 0, p(out)) == -1
    assert rb(ctx.h, C.byref(req), p(data), data.size, -2, ok, 2, 0, p(out)) == -1
    assert rb(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, None) == -1
    assert rb(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, vp(out.ctypes.data + 4)) == -1
    for bands, count in bad_bands:
        assert rb(ctx.h, C.byref(req), p(data), data.size, width, bands, count, 0, p(out)) == -1, count
    assert (out == 0).all()
    req16, keep16 = pkg.binding._make_request(pkg.parse_format("CS16")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False)
    assert rb(ctx.h, C.byref(req16), p(data), 4 * 100 + 1, width, ok, 2, 0, p(out)) == -3
    assert rb(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, p(out)) == 0
    got = out[:2 * width].reshape(2, width)
    assert np.isfinite(got).all() and (got[0] > got[1]).all() and (got[1] > 0).all() and (out[2 * width:] == 0).all()


# ---- (g) interleaving -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width", [("CS16", 256, 300), ("CU8", 2048, 37)])
def test_execute_and_execute_bandpower_interleave_without_a_synchronisation(ctx, fmt, n, width):
    data, win, bn, _, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want, bands = _want(fmt, n, width, False, n // 2 + 3), bandref.standard_bands(n)
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    r_want = pyoracle.render(fmt, data, n, win, bn, 3.0, 50.0, lut, width)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, lut)
    d_in = _upload(ctx, data)
    sizes = [4 * width * n, width, width, width, 8 * 256, 8000, 16]
    first = [ctx.alloc(s_) for s_ in sizes]
    second = [ctx.alloc(s_) for s_ in sizes]
    out = _Out(ctx, len(bands), width)

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
        plan.execute_bandpower(d_in, data.size, width, bands, out.ptr)
        plan.execute(d_in, data.size, width, *second)
        ctx.synchronize()
        assert_same_reply(reply(first), r_want)
        assert_same_reply(reply(second), r_want)
        bandref.assert_same(out.read("interleaved"), want, "interleaved")
    finally:
        out.free()
        for p_ in first + second + [d_in]:
            ctx.free(p_)
        plan.close()
