"""The exact spectral moments on the GPU (sp_power_moments, sp_plan_execute_moments, sp_render_moments): every comparison is bit for bit
against tests/momentref.py - exact rational sums rounded once - on a synthetic plane or on the oracle's plane (tests/powerref.py, the
references of tests/test_mean_gpu.py shared); which NaN a NaN is, is the one thing left uncompared.  Every result lies between guard
bytes and holds garbage before the call.

The measurement that goes with the feature is not asserted here (tools/moment_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bandref
import meanref
import momentref
import powerref
from __graft_entry__ import load_package
from oracle import pyoracle
from test_gpu_parity import _assert_same as assert_same_reply
from test_mean_gpu import GARBAGE, GUARD, _capture, _reference, _upload

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
    """A device array f64 of `shape` between two guards, everything garbage."""

    def __init__(self, ctx, *shape):
        self.ctx, self.shape, self.bytes = ctx, shape, 8 * int(np.prod(shape))
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


def _power_moments(ctx, plane, bands, order, what):
    """sp_power_moments of a host plane f64 [width, n] through a device copy."""
    width, n = plane.shape
    d_p, out = _upload(ctx, plane), _Out(ctx, order + 1, len(bands), width)
    try:
        ctx.power_moments(d_p if width else 0, n, width, bands, order, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_p)
        out.free()


def _power_bands(ctx, plane, bands):
    width, n = plane.shape
    d_p, out = _upload(ctx, plane), _Out(ctx, len(bands), width)
    try:
        ctx.power_bands(d_p, n, width, bands, out.ptr)
        ctx.synchronize()
        return out.read("sp_power_bands")
    finally:
        ctx.free(d_p)
        out.free()


def _execute_moments(ctx, plan, d_in, nbytes, width, bands, order, what):
    out = _Out(ctx, order + 1, len(bands), width)
    try:
        plan.execute_moments(d_in, nbytes, width, bands, order, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- (a) sp_power_moments on synthetic planes ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(n, width):
    plane = bandref.synthetic_plane(7000 * n + width, n, width)
    plane.setflags(write=False)
    want = momentref.expected(plane, bandref.standard_bands(n))
    want.setflags(write=False)
    return plane, want


@pytest.mark.parametrize("width", [1, 2, 7, 8, 9, 65])
@pytest.mark.parametrize("n", [2, 64, 100, 256])
def test_power_moments_of_synthetic_planes(ctx, n, width):
    """Frames over the full exponent range (64 values of a load in up to 64 different cells), denormals, cell-boundary exponents, ties
    at 2^53 and a frame of DBL_MAX; n = 100 is no multiple of a load's 64 rows, the widths are below, at and past a workgroup's 8
    frames.  m[0] is sp_power_bands' series bit for bit."""
    plane, want = _synthetic(n, width)
    bands = bandref.standard_bands(n)
    what = "sp_power_moments n=%d W=%d" % (n, width)
    got = _power_moments(ctx, plane, bands, 2, what)
    momentref.assert_same(got, want, what)
    sums = _power_bands(ctx, plane, bands)
    nan = np.isnan(sums)
    assert np.array_equal(np.isnan(got[0]), nan) and np.array_equal(_bits(got[0])[~nan], _bits(sums)[~nan])
    assert (_bits(got[:, 0]) == 0).all()                                        # the empty band: +0.0 in every moment
    assert (_bits(got[1:, 1]) == 0).all() and (_bits(got[1:, 5]) == 0).all()    # a band of one row: m1 = m2 = +0.0
    assert np.array_equal(_bits(got[0, 1]), _bits(plane[:, 0].copy()))          # ... and m0 the plane's column


@pytest.mark.parametrize("order", [0, 1])
def test_a_lower_order_is_the_same_series(ctx, order):
    n, width = 100, 9
    plane, want = _synthetic(n, width)
    got = _power_moments(ctx, plane, bandref.standard_bands(n), order, "order %d" % order)
    assert got.shape == (order + 1, 8, width)
    momentref.assert_same(got, want[:order + 1], "order %d" % order)


WALK_BANDS = [(0, 700), (3, 324), (255, 257), (256, 512), (699, 700), (5, 5)]


@functools.lru_cache(maxsize=None)
def _walk():
    n, width = 700, 9
    plane = bandref.synthetic_plane(7000 * n + width, n, width)
    plane.setflags(write=False)
    want = momentref.expected(plane, WALK_BANDS)
    want.setflags(write=False)
    return plane, want


@pytest.mark.parametrize("order", [0, 1, 2])
def test_the_walk_past_one_step_of_rows_at_every_order(ctx, order):
    """The kernel of every order walks a band 64 x 4 rows at a time: n = 700 gives a band of three steps whose last load is partial, a
    start off a multiple of 64, a band across a step's edge, one that begins at one, one row and no row; W = 9 leaves the last
    workgroup one frame.  m[0] of every order is sp_power_bands' series bit for bit."""
    plane, want = _walk()
    what = "sp_power_moments n=700 W=9 order %d" % order
    got = _power_moments(ctx, plane, WALK_BANDS, order, what)
    assert got.shape == (order + 1, len(WALK_BANDS), 9)
    momentref.assert_same(got, want[:order + 1], what)
    sums = _power_bands(ctx, plane, WALK_BANDS)
    nan = np.isnan(sums)
    assert np.array_equal(np.isnan(got[0]), nan) and np.array_equal(_bits(got[0])[~nan], _bits(sums)[~nan])


@functools.lru_cache(maxsize=None)
def _largest():
    """n = 2^20, two frames: a dense spectrum-like frame (clustered exponents) and a frame of a few thousand values over a wide range
    of exponents with one in the last row - the largest weight - none so large that the moments overflow."""
    n = 1 << 20
    rng = np.random.default_rng(2 ** 20)
    plane = np.zeros((2, n))
    plane[0] = meanref.random_values(rng, n, clustered=True)
    rows = np.unique(np.concatenate([rng.integers(0, n, 4000), np.arange(n - 70, n), [0, 1, 63, 64]]))
    plane[1, rows] = meanref._from_fields(rng, rng.integers(0, 1900, rows.size), rows.size)
    bands = [(0, n), (n - 65, n)]
    want = np.zeros((3, 2, 2))
    for x in range(2):
        want[:, 0, x] = momentref.dense_column(plane[x])
        want[:, 1, x] = momentref.column(plane[x, n - 65:])
    assert np.isfinite(want).all() and (want > 0).all()
    return plane, bands, want


def test_power_moments_at_the_largest_n(ctx):
    """The plane is 16 MiB; the last row of the whole band has the weight (2^20 - 1)^2."""
    plane, bands, want = _largest()
    momentref.assert_same(_power_moments(ctx, plane, bands, 2, "n = 2^20"), want, "sp_power_moments at n = 2^20")


def test_power_moments_with_the_most_bands(ctx):
    n, width = 100, 65
    plane = _synthetic(n, width)[0]
    bands = [(k, min(n, k + k % 7)) for k in range(bandref.SP_MAX_BANDS)]
    assert len(bands) == 64 and any(y0 == y1 for y0, y1 in bands)
    momentref.assert_same(_power_moments(ctx, plane, bands, 2, "64 bands"), momentref.expected(plane, bands), "sp_power_moments with 64 bands")


def test_special_values_are_the_bands(ctx):
    n, width = 100, 9
    plane = _synthetic(n, width)[0].copy()
    plane[1, 0] = np.inf              # +inf in the row of weight 0 of the bands that begin at row 0
    plane[2, 0] = np.nan              # a NaN there
    plane[3, 70] = np.inf
    plane[3, 71] = np.nan             # NaN beats inf
    plane[4, 10] = np.nan
    plane[8, 99] = np.inf             # the last frame's last row
    bands = bandref.standard_bands(n) + [(0, 1), (10, 11), (11, 71), (70, 72), (71, 100)]
    want = momentref.expected(plane, bands)
    assert np.isinf(want[:, 2, 1]).all() and np.isinf(want[:, 8, 1]).all() and np.isnan(want[:, 2, 2]).all() and np.isnan(want[:, 8, 2]).all()
    assert np.isnan(want[:, 2, 3]).all() and np.isinf(want[:, 10, 3]).all() and np.isnan(want[:, 11, 3]).all() and np.isfinite(want[:, 9, 3]).all()
    assert np.isinf(want[:, 5, 8]).all() and np.isfinite(want[:, 5, 7]).all()
    momentref.assert_same(_power_moments(ctx, plane, bands, 2, "specials"), want, "sp_power_moments specials")


# ---- (b) sp_plan_execute_moments against the oracle's plane: the window, the interleaving --------------------------------------------------
ORACLE = [("CF32", 64, 37, False, "frames_power"), ("CS16", 1024, 37, False, "frames_power"), ("CF32", 2048, 2, False, "scratch_power")]


@functools.lru_cache(maxsize=None)
def _want(fmt, n, width, ch, stride, bands=None):
    """The moments of the bands (default: bandref.standard_bands(n)) over the plane test_mean_gpu's reference holds for this request."""
    plane = _reference(fmt, n, width, ch, stride)[3]
    want = momentref.expected(plane, list(bands) if bands else bandref.standard_bands(n))
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("fmt,n,width,ch,name", ORACLE, ids=["n%d" % c[1] for c in ORACLE])
def test_execute_moments_against_the_oracle_whatever_the_window(ctx, fmt, n, width, ch, name):
    data, win, bn, plane, _ = _reference(fmt, n, width, ch, n // 2 + 3)
    want, bands = _want(fmt, n, width, ch, n // 2 + 3), bandref.standard_bands(n)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    got = []
    try:
        assert plan.moments_kernel_name_for(data.size, width) == name + "+moments"
        for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, below one frame (one frame), the default
            ctx.set_mean_window(window)
            got.append(_execute_moments(ctx, plan, d_in, data.size, width, bands, 2, "window %d" % window))
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()
    for g in got:
        momentref.assert_same(g, want, "%s n=%d W=%d" % (fmt, n, width))
        assert np.array_equal(_bits(g), _bits(got[0]))
    m0, m1, m2 = got[0]
    assert np.array_equal(_bits(m0[5]), _bits(plane[:, n - 1].copy()))
    assert (m0[2] > 0).all() and (m1[2] > 0).all() and (m1[2] < m0[2] * n).all() and (m2[2] < m1[2] * n).all()      # 0 <= y - y0 < n


def test_execute_moments_interleaves_without_a_synchronisation(ctx):
    fmt, n, width = "CS16", 1024, 37
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
    out, sums = _Out(ctx, 3, len(bands), width), _Out(ctx, len(bands), width)

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
        plan.execute_moments(d_in, data.size, width, bands, 2, out.ptr)
        plan.execute_bandpower(d_in, data.size, width, bands, sums.ptr)
        plan.execute(d_in, data.size, width, *second)
        ctx.synchronize()
        assert_same_reply(reply(first), r_want)
        assert_same_reply(reply(second), r_want)
        got = out.read("interleaved")
        momentref.assert_same(got, want, "interleaved")
        assert np.array_equal(_bits(got[0]), _bits(sums.read("interleaved band sums")))
    finally:
        out.free()
        sums.free()
        for p_ in first + second + [d_in]:
            ctx.free(p_)
        plan.close()


# ---- (c) the host entry point -------------------------------------------------------------------------------------------------------------------
def _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands, order=2, ch=False, db=0, detector="sample"):
    """sp_render_moments into a host array between guards, everything garbage: (status, the moments, nothing but them was written)."""
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, ch, False, detector)
    b = np.ascontiguousarray(np.asarray(bands, np.int32).reshape(-1, 2))
    count, series = b.shape[0], max(order, 0) + 1
    size = 8 * series * count * max(width, 0)
    host = np.full(size + 2 * GUARD, GARBAGE, np.uint8)
    vp = C.c_void_p
    rc = ctx.lib.L.sp_render_moments(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, width, b.ctypes.data_as(vp) if count else None,
                                     count, order, db, vp(host.ctypes.data + GUARD))
    intact = bool((host[:GUARD] == GARBAGE).all() and (host[GUARD + size:] == GARBAGE).all())
    return rc, host[GUARD:GUARD + size].view(np.float64).reshape(series, count, max(width, 0)).copy(), intact, host


def test_dense_render_moments_and_the_db_form(pkg, ctx):
    fmt, n, width = "CF32", 64, 37
    data, win, bn, _, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want, bands = _want(fmt, n, width, False, n // 2 + 3), bandref.standard_bands(n)
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands)
    assert rc == 0 and intact
    momentref.assert_same(got, want, "dense sp_render_moments")
    momentref.assert_same(ctx.render_moments(fmt, data, n, win, bn, 3.0, 50.0, width, bands, 2, fill=GARBAGE), want, "Context.render_moments")
    assert ctx.render_moments(fmt, data, n, win, bn, 3.0, 50.0, width, bands, fill=GARBAGE).shape == (2, len(bands), width)   # order 1
    # db = 1 converts m[0] exactly as sp_plan_power_to_db does, and m[1] and m[2] are untouched
    rc, got_db, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands, db=1)
    assert rc == 0 and intact
    want_db = meanref.db_of(want[0].reshape(-1), bn, 3.0).reshape(want[0].shape)
    bandref.assert_same(got_db[0], want_db, "the dB form of m[0] against the oracle's log10")
    assert np.array_equal(_bits(got_db[1:]), _bits(got[1:]))
    host_db = ctx.render_bandpower(fmt, data, n, win, bn, 3.0, 50.0, width, bands, db=True, fill=GARBAGE)
    assert np.array_equal(_bits(host_db), _bits(got_db[0]))
    assert np.isneginf(got_db[0, 0]).all() and np.isfinite(got_db[0, 2]).all()


def test_small_sparse_request_uploads_its_frames_only(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, _ = _reference(fmt, n, width, False, 40 * n + 11)
    want, bands = _want(fmt, n, width, False, 40 * n + 11), bandref.standard_bands(n)
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands)
    assert rc == 0 and intact
    momentref.assert_same(got, want, "sparse sp_render_moments")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1


def test_chunked_sp_render_moments(pkg, ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts: the capture travels in chunks and every chunk fills its columns of
    every series.  (Narrow bands: the reference is rational arithmetic over 2048 frames.)"""
    fmt, n, width = "CF32", 1024, 2048
    bands = ((500, 520), (0, 1), (n - 2, n), (3, 3))
    data, win, bn, _, _ = _reference(fmt, n, width, False, n)
    want = _want(fmt, n, width, False, n, bands)
    assert data.size >= 16 << 20
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands)
    assert rc == 0 and intact
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    momentref.assert_same(got, want, "chunked sp_render_moments")


# ---- (d) nothing to write, and refusals ---------------------------------------------------------------------------------------------------------
def test_width_0_and_count_0_write_nothing(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, _ = _reference(fmt, n, width, False, 40 * n + 11)
    for w, bands in ((0, [(0, n), (3, 9)]), (width, [])):
        rc, _, intact, host = _render_guarded(ctx, pkg, fmt, data, n, win, bn, w, bands)
        assert rc == 0 and intact and (host == GARBAGE).all()
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in, d_plane, out = _upload(ctx, data), ctx.alloc(8 * width * n), _Out(ctx, 1)
    try:
        for order in (0, 2):
            plan.execute_moments(d_in, data.size, 0, [(0, n)], order, out.ptr)
            plan.execute_moments(d_in, data.size, width, [], order, out.ptr)
            plan.execute_moments(d_in, data.size, width, [], order, 0)
            ctx.power_moments(d_plane, n, 0, [(0, n)], order, out.ptr)
            ctx.power_moments(d_plane, n, width, [], order, out.ptr)
            ctx.power_moments(0, n, 0, [(0, n)], order, 0)
        ctx.synchronize()
        assert (out.whole() == GARBAGE).all()
    finally:
        out.free()
        for p in (d_in, d_plane):
            ctx.free(p)
        plan.close()


def test_refusals_write_nothing(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    vp = C.c_void_p
    d_in, d_plane, out = _upload(ctx, data), ctx.alloc(8 * width * n + 16), _Out(ctx, 3, 64, width)

    def arr(*rows):
        return (C.c_int32 * len(rows))(*rows)

    ok, many = arr(0, n, 3, 9), arr(*([0, 1] * 65))
    bad_bands = [(arr(0, n + 1), 1), (arr(-1, 4), 1), (arr(5, 4), 1), (arr(0, n, n + 1, n + 1), 2), (many, 65), (ok, -1), (None, 1)]
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        ctx.memset(d_plane, 0, 8 * width * n + 16)
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_moments(d_in, data.size, width, [(0, n)], 2, out.ptr)
        assert e.value.status == -4 and "peak" in str(e.value)               # the band-power series' status for a peak plan
        ex, pm = L.sp_plan_execute_moments, L.sp_power_moments
        assert ex(None, vp(d_in), data.size, width, ok, 2, 2, vp(out.ptr)) == -1
        assert pm(None, vp(d_plane), n, width, ok, 2, 2, vp(out.ptr)) == -1
        for order in (-1, 3, 1 << 30):
            assert ex(plan.h, vp(d_in), data.size, width, ok, 2, order, vp(out.ptr)) == -1, order
            assert pm(ctx.h, vp(d_plane), n, width, ok, 2, order, vp(out.ptr)) == -1, order
        for bands, count in bad_bands:
            assert ex(plan.h, vp(d_in), data.size, width, bands, count, 2, vp(out.ptr)) == -1, count
            assert pm(ctx.h, vp(d_plane), n, width, bands, count, 2, vp(out.ptr)) == -1, count
        for bad_out in (None, vp(out.ptr + 4)):                              # NULL, misaligned
            assert ex(plan.h, vp(d_in), data.size, width, ok, 2, 2, bad_out) == -1
            assert pm(ctx.h, vp(d_plane), n, width, ok, 2, 2, bad_out) == -1
        assert ex(plan.h, vp(d_in), data.size, -1, ok, 2, 2, vp(out.ptr)) == -1
        assert ex(plan.h, None, data.size, width, ok, 2, 2, vp(out.ptr)) == -1
        assert pm(ctx.h, vp(d_plane), 0, width, arr(0, 0), 1, 2, vp(out.ptr)) == -1
        assert pm(ctx.h, vp(d_plane), (1 << 20) + 1, width, ok, 2, 2, vp(out.ptr)) == -1     # a weight would pass 2^40
        assert pm(ctx.h, vp(d_plane + 4), n, width, ok, 2, 2, vp(out.ptr)) == -1
        assert pm(ctx.h, None, n, width, ok, 2, 2, vp(out.ptr)) == -1
        ctx.synchronize()
        assert (out.whole() == GARBAGE).all()
        assert ex(plan.h, vp(d_in), data.size, width, many, 64, 2, vp(out.ptr)) == 0          # 64 bands are allowed
        ctx.synchronize()
        got = out.read("64 bands")
        assert np.isfinite(got[0]).all() and (_bits(got[1:]) == 0).all()                      # bands of one row
    finally:
        peak.close()
        plan.close()
        out.free()
        for p_ in (d_in, d_plane):
            ctx.free(p_)
    # the host entry
    bands = [(0, n), (3, 9)]
    for kw in ({"detector": "peak"}, {"order": -1}, {"order": 3}):
        rc, _, intact, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, bands, **kw)
        assert rc == (-4 if "detector" in kw else -1) and (host == GARBAGE).all(), kw
    for bad in ([(0, n + 1)], [(-1, 4)], [(5, 4)], [(0, 1)] * 65):
        rc, _, intact, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, bad)
        assert rc == -1 and (host == GARBAGE).all(), bad
    rc, got, intact, _ = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, bands)
    assert rc == 0 and intact and np.isfinite(got).all() and (got[0, 0] > got[0, 1]).all() and (got[:, 1] > 0).all()
