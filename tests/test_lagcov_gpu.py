"""The exact lagged covariances of band-power series on the GPU (sp_series_lagcov, sp_power_lagcov, sp_plan_execute_lagcov,
sp_render_lagcov): every comparison is bit for bit against tests/lagcovref.py - integer products, sums and their signed difference,
rounded once - on synthetic series or on the band sums (tests/bandref.py) of the oracle's plane (tests/powerref.py, the references of
tests/test_mean_gpu.py shared); which NaN a NaN is, is the one thing left uncompared.  Every reply lies between guard bytes and holds
garbage before the call.

The shapes are the smallest at which the kernel can go wrong: the lag-band edges (32 lags to a workgroup), and term counts at a piece
edge (32 terms), one round of 8 streams of 4 loads, and several pieces.  The measurement that goes with the feature is not asserted
here (tools/lagcov_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bandref
import lagcovref
import meanref
import powerref
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle
from test_gpu_parity import _assert_same as assert_same_reply
from test_mean_gpu import GARBAGE, GEN, GUARD, _capture, _reference, _upload

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
    """A device array f64 [3, npairs, lags] between two guards, everything garbage."""

    def __init__(self, ctx, npairs, lags):
        self.ctx, self.shape, self.bytes = ctx, (3, npairs, lags), 24 * npairs * lags
        self.base = ctx.alloc(self.bytes + 2 * GUARD)
        assert self.base % 8 == 0
        self.ptr = self.base + GUARD
        ctx.memset(self.base, GARBAGE, self.bytes + 2 * GUARD)

    def whole(self):
        return self.ctx.download(self.base, self.bytes + 2 * GUARD)

    def read(self, what=""):
        whole = self.whole()
        assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + self.bytes:] == GARBAGE).all(), what + ": bytes around the reply were written"
        return whole[GUARD:GUARD + self.bytes].view(np.float64).reshape(self.shape).copy()

    def free(self):
        self.ctx.free(self.base)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _series_lagcov(ctx, series, pairs, lags, what):
    """sp_series_lagcov of a host series f64 [count, width] through a device copy."""
    count, width = series.shape
    d_s, out = _upload(ctx, series), _Out(ctx, len(pairs), lags)
    try:
        ctx.series_lagcov(d_s if series.size else 0, count, width, pairs, lags, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_s)
        out.free()


# ---- (a) sp_series_lagcov on synthetic series: lags and terms swept --------------------------------------------------------------------
SWEEP_PAIRS = [(0, 0), (0, 1), (2, 1)]


@functools.lru_cache(maxsize=None)
def _sweep(lags, terms):
    width = terms + lags - 1 if terms else lags - 1
    series = lagcovref.synthetic_series(100 * lags + terms, 3, width)
    want = lagcovref.expected(series, SWEEP_PAIRS, lags)
    for a in (series, want):
        a.setflags(write=False)
    return series, want


@pytest.mark.parametrize("terms", [0, 1, 2, 33, 257, 1031])
@pytest.mark.parametrize("lags", [1, 2, 31, 32, 33, 65])
def test_series_lagcov_over_lag_bands_and_pieces(pkg, ctx, lags, terms):
    """lags: below, at and past one and two bands of 32 lags.  N: none, one, two, past a 32-term piece, past one round of 8 streams of 4
    loads several times over, and several pieces at any CU count.  An auto pair on a pedestal, a cross pair whose covariance is
    negative, and a pair with the full exponent range."""
    series, want = _sweep(lags, terms)
    assert pkg.lagcov_terms(series.shape[1], lags) == terms
    what = "sp_series_lagcov lags=%d N=%d" % (lags, terms)
    got = _series_lagcov(ctx, series, SWEEP_PAIRS, lags, what)
    lagcovref.assert_same(got, want, what)
    if terms == 0:
        assert (_bits(got) == 0).all()
    if terms >= 33:
        assert got[1, 0, 0] > 0 and got[1, 1, 0] < 0 and np.isfinite(got[:, :2]).all()      # the pedestal pairs: exact, and signed


# ---- (b) pairs and values ----------------------------------------------------------------------------------------------------------------
def _many_pairs(npairs):
    base = [(0, 0), (0, 1), (1, 0), (2, 2), (2, 3), (3, 2), (4, 5), (5, 4), (4, 4), (5, 5), (3, 3), (1, 1), (0, 5), (4, 0), (2, 0), (3, 1)]
    return base[:npairs]


@functools.lru_cache(maxsize=None)
def _valued(npairs):
    lags, terms = 33, 257
    width = terms + lags - 1
    series = lagcovref.synthetic_series(7 + npairs, 6, width)
    # window edges: a's window is [0, N), b's at lag l is [l, l + N)
    series[0, terms] = np.nan              # outside a's window: marks (., 0) pairs at the lags >= 1 only
    series[1, 0] = np.inf                  # marks (1, .) at every lag and (., 1) at lag 0 only
    series[4, terms - 1] = np.inf          # the last frame of a's window; in b's at every lag
    series[5, width - 1] = np.nan          # b's window at the last lag only
    pairs = _many_pairs(npairs)
    want = lagcovref.expected(series, pairs, lags)
    for a in (series, want):
        a.setflags(write=False)
    return series, pairs, lags, want


@pytest.mark.parametrize("npairs", [1, 3, 16])
def test_series_lagcov_pairs_and_values(ctx, npairs):
    """Auto pairs, cross pairs and their reverses over six series: a pedestal and its complement, the full exponent range, denormals
    with zeros, and clusters at 1e-150 and 1e150 whose products reach both ends of the cells; a NaN and an inf at window edges."""
    series, pairs, lags, want = _valued(npairs)
    what = "sp_series_lagcov npairs=%d" % npairs
    got = _series_lagcov(ctx, series, pairs, lags, what)
    lagcovref.assert_same(got, want, what)
    assert np.isfinite(got[:, 0, 0]).all() and np.isnan(got[:, 0, 1:]).all()                # (0, 0): the NaN at a[N] is b's from lag 1 on
    if npairs >= 3:
        assert np.isinf(got[:, 1, 0]).all() and np.isfinite(got[:, 1, 1:]).all()            # (0, 1): the inf at b[0] is lag 0's alone
        assert np.isinf(got[:, 2, 0]).all() and np.isnan(got[:, 2, 1:]).all()               # (1, 0): the inf at a[0], and NaN beats it
    if npairs == 16:
        assert np.array_equal(_bits(got[:2, 4, 0]), _bits(got[:2, 5, 0]))                   # lag 0 of (2, 3) and of (3, 2): the same bits
        assert np.isinf(got[:, 8]).all() and np.isnan(got[:, 9, lags - 1]).all() and np.isfinite(got[:, 9, :lags - 1]).all()
        assert np.isfinite(got[:, 10]).all() and np.signbit(got[1]).any()


# ---- (c) sp_power_lagcov is sp_power_bands followed by sp_series_lagcov ----------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 64, 100])
def test_power_lagcov_is_power_bands_then_series_lagcov(ctx, n):
    width, lags = 70, 9
    plane = np.ascontiguousarray(meanref.synthetic_plane(500 + n, width, n))
    bands = [(0, 1), (0, n), (n // 2, n)]
    pairs = [(0, 0), (1, 2), (2, 1), (0, 1)]
    d_p, d_s = _upload(ctx, plane), ctx.alloc(8 * len(bands) * width)
    direct, chained = _Out(ctx, len(pairs), lags), _Out(ctx, len(pairs), lags)
    try:
        ctx.power_lagcov(d_p, n, width, bands, pairs, lags, direct.ptr)
        ctx.power_bands(d_p, n, width, bands, d_s)
        ctx.series_lagcov(d_s, len(bands), width, pairs, lags, chained.ptr)
        ctx.synchronize()
        a, b = direct.read("sp_power_lagcov"), chained.read("sp_series_lagcov")
        series = ctx.download(d_s, 8 * len(bands) * width, np.float64).reshape(len(bands), width)
    finally:
        direct.free()
        chained.free()
        for p_ in (d_p, d_s):
            ctx.free(p_)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])
    bandref.assert_same(series, bandref.expected(plane, bands), "sp_power_bands n=%d" % n)
    lagcovref.assert_same(a, lagcovref.expected(series, pairs, lags), "sp_power_lagcov n=%d" % n)
    bandref.assert_same(series[:1], plane[:, 0][None, :], "a single-row band is the row, bit for bit")


# ---- (d) the variance cross-check on the device ----------------------------------------------------------------------------------------
def test_a_single_row_at_lag_zero_is_the_variance(ctx):
    n, width = 64, 257
    import varianceref
    plane = varianceref.synthetic_plane(4242, width, n)
    d_p, d_v = _upload(ctx, plane), ctx.alloc(24 * n)
    out = _Out(ctx, 1, 1)
    try:
        ctx.power_variance(d_p, n, width, d_v)
        ctx.synchronize()
        var = ctx.download(d_v, 24 * n, np.float64).reshape(3, n)
        for y in (0, 7, 8, 9, 13, 14, 15, 20, 63):      # plain rows, the constant row, one ulp, DBL_MAX in one frame, NaN, inf, both
            ctx.memset(out.base, GARBAGE, out.bytes + 2 * GUARD)
            ctx.power_lagcov(d_p, n, width, [(y, y + 1)], [(0, 0)], 1, out.ptr)
            ctx.synchronize()
            got = out.read("row %d" % y)[:, 0, 0]
            lagcovref.assert_same(got, np.array([var[1, y], var[2, y], var[0, y]]), "row %d against sp_power_variance" % y)
    finally:
        out.free()
        for p_ in (d_p, d_v):
            ctx.free(p_)


# ---- (e) sp_plan_execute_lagcov and sp_render_lagcov against the oracle's plane --------------------------------------------------------
def _bands(n):
    return [(0, n), (n // 4, n // 2), (n // 2, n // 2 + 1), (1, 3)]


PAIRS = [(0, 0), (1, 2), (2, 1), (3, 3)]


@functools.lru_cache(maxsize=None)
def _want(fmt, n, width, stride, lags):
    """The reply for the band sums of the plane test_mean_gpu's reference holds for this request."""
    series = bandref.expected(_reference(fmt, n, width, False, stride)[3], _bands(n))
    want = lagcovref.expected(series, PAIRS, lags)
    want.setflags(write=False)
    return want


def _execute_lagcov(ctx, plan, d_in, nbytes, width, n, lags, what):
    out = _Out(ctx, len(PAIRS), lags)
    try:
        plan.execute_lagcov(d_in, nbytes, width, _bands(n), PAIRS, lags, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


ORACLE = [("CF32", 64, 37, False, "frames_power"), ("CS16", 1024, 37, False, "frames_power"), ("CF32", 64, 37, True, "scratch_power"),
          ("CF32", 2048, 2, False, "scratch_power")]


@pytest.mark.parametrize("fmt,n,width,forced,name", ORACLE, ids=["n%d%s" % (c[1], "-forced" if c[3] else "") for c in ORACLE])
def test_execute_lagcov_against_the_oracle_whatever_the_window(ctx, fmt, n, width, forced, name):
    lags = 5 if width > 5 else 2
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want = _want(fmt, n, width, n // 2 + 3, lags)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, data)
    got = []
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.lagcov_kernel_name_for(data.size, width) == name + "+lagcov"
        for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, below one frame (one frame), the default
            ctx.set_mean_window(window)
            got.append(_execute_lagcov(ctx, plan, d_in, data.size, width, n, lags, "window %d" % window))
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()
    for g in got:
        lagcovref.assert_same(g, want, "%s n=%d W=%d" % (fmt, n, width))
        assert np.array_equal(_bits(g), _bits(got[0]))
    assert np.isfinite(got[0]).all() and (got[0][0] > 0).all() and (got[0][2] > 0).all()
    assert np.array_equal(_bits(got[0][:2, 1, 0]), _bits(got[0][:2, 2, 0]))                 # lag 0 of (1, 2) and of (2, 1)


def test_execute_lagcov_interleaves_without_a_synchronisation(ctx):
    import varianceref
    fmt, n, width, lags = "CS16", 1024, 37, 5
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want = _want(fmt, n, width, n // 2 + 3, lags)
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    r_want = pyoracle.render(fmt, data, n, win, bn, 3.0, 50.0, lut, width)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, lut)
    d_in = _upload(ctx, data)
    sizes = [4 * width * n, width, width, width, 8 * 256, 8000, 16]
    first = [ctx.alloc(s_) for s_ in sizes]
    second = [ctx.alloc(s_) for s_ in sizes]
    bands = _bands(n)
    d_band, d_var = ctx.alloc(8 * len(bands) * width), ctx.alloc(24 * n)
    out, again = _Out(ctx, len(PAIRS), lags), _Out(ctx, len(PAIRS), lags)

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
        plan.execute_lagcov(d_in, data.size, width, bands, PAIRS, lags, out.ptr)
        plan.execute_bandpower(d_in, data.size, width, bands, d_band)
        plan.execute_variance(d_in, data.size, width, d_var)
        plan.execute_lagcov(d_in, data.size, width, bands, PAIRS, lags, again.ptr)
        plan.execute(d_in, data.size, width, *second)
        ctx.synchronize()
        assert_same_reply(reply(first), r_want)
        assert_same_reply(reply(second), r_want)
        lagcovref.assert_same(out.read("interleaved"), want, "interleaved")
        lagcovref.assert_same(again.read("interleaved, again"), want, "interleaved, again")
        bandref.assert_same(ctx.download(d_band, 8 * len(bands) * width, np.float64).reshape(len(bands), width),
                            bandref.expected(plane, bands), "interleaved bandpower")
        varianceref.assert_same(ctx.download(d_var, 24 * n, np.float64).reshape(3, n), varianceref.expected(plane), "interleaved variance")
    finally:
        out.free()
        again.free()
        for p_ in first + second + [d_in, d_band, d_var]:
            ctx.free(p_)
        plan.close()


def _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, lags, detector="sample", bands=None, pairs=PAIRS):
    """sp_render_lagcov into a host array between guards, everything garbage: (status, the reply, nothing but it was written, the whole
    array)."""
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, False, False, detector)
    b = np.ascontiguousarray(np.asarray(_bands(n) if bands is None else bands, np.int32).reshape(-1, 2))
    p = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    shape = (3, len(p), max(lags, 0))
    size = 24 * shape[1] * shape[2]
    host = np.full(size + 2 * GUARD, GARBAGE, np.uint8)
    vp = C.c_void_p
    rc = ctx.lib.L.sp_render_lagcov(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, width, b.ctypes.data_as(vp), len(b),
                                    p.ctypes.data_as(vp), len(p), lags, vp(host.ctypes.data + GUARD))
    intact = bool((host[:GUARD] == GARBAGE).all() and (host[GUARD + size:] == GARBAGE).all())
    return rc, host[GUARD:GUARD + size].view(np.float64).reshape(shape).copy(), intact, host


def test_dense_render_lagcov(pkg, ctx):
    fmt, n, width, lags = "CF32", 64, 37, 5
    data, win, bn, _, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want = _want(fmt, n, width, n // 2 + 3, lags)
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, lags)
    assert rc == 0 and intact
    lagcovref.assert_same(got, want, "dense sp_render_lagcov")
    lagcovref.assert_same(ctx.render_lagcov(fmt, data, n, win, bn, 3.0, 50.0, width, _bands(n), PAIRS, lags, fill=GARBAGE), want,
                          "Context.render_lagcov")


def test_small_sparse_request_uploads_its_frames_only(pkg, ctx):
    fmt, n, width, lags = "CU8", 256, 64, 9
    data, win, bn, _, _ = _reference(fmt, n, width, False, 40 * n + 11)
    want = _want(fmt, n, width, 40 * n + 11, lags)
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, lags)
    assert rc == 0 and intact
    lagcovref.assert_same(got, want, "sparse sp_render_lagcov")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1


def test_chunked_sp_render_lagcov(pkg, ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts: the capture travels in chunks, every chunk's blocks write their columns
    of the workspace series, and the lags reach across the chunk edges."""
    fmt, n, width, lags = "CF32", 1024, 2048, 5
    data, win, bn, _, _ = _reference(fmt, n, width, False, n)
    want = _want(fmt, n, width, n, lags)
    assert data.size >= 16 << 20
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, lags)
    assert rc == 0 and intact
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    lagcovref.assert_same(got, want, "chunked sp_render_lagcov")


# ---- (f) no frames, and refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 2048])
def test_a_capture_shorter_than_n_and_a_request_of_no_terms(pkg, ctx, n):
    """A capture shorter than n: the oracle's plane is NaN in every frame, so is the series, and so is the reply.  N = 0 - no frames, or
    fewer frames than lags - writes 3 * npairs * lags times +0.0."""
    data = siggen.generate("CS16", GEN, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    plane = powerref.expected("CS16", data, n, win, 1.0 / weight, 3.0, 50.0, 3, False)["power"]
    want = lagcovref.expected(bandref.expected(plane, _bands(n)), PAIRS, 2)
    assert np.isnan(want).all()
    rc, got, intact, _ = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, 3, 2)
    assert rc == 0 and intact
    lagcovref.assert_same(got, want, "a capture shorter than n")
    for width, lags in ((0, 1), (0, 3), (3, 4)):
        rc, got, intact, _ = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, width, lags)
        assert rc == 0 and intact and (_bits(got) == 0).all(), (width, lags)
    long = _capture("CS16", n, 4, n)
    plan = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, long)
    try:
        for width, lags in ((0, 2), (4, 5)):
            got = _execute_lagcov(ctx, plan, d_in, long.size, width, n, lags, "N = 0")
            assert (_bits(got) == 0).all()
    finally:
        ctx.free(d_in)
        plan.close()


def test_refusals_write_nothing(pkg, ctx):
    n, width, lags = 128, 20, 3
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    vp = C.c_void_p
    i32 = lambda v: np.ascontiguousarray(np.asarray(v, np.int32).reshape(-1))  # noqa: E731
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    bands, pairs = i32([0, n, 3, 9]), i32([0, 1, 1, 1])
    d_in, d_plane, out = _upload(ctx, data), ctx.alloc(8 * width * n + 16), _Out(ctx, 2, lags)
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        ctx.memset(d_plane, 0, 8 * width * n + 16)
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_lagcov(d_in, data.size, width, [(0, n), (3, 9)], [(0, 1), (1, 1)], lags, out.ptr)
        assert e.value.status == -4 and "peak" in str(e.value)
        ex, pw, se = L.sp_plan_execute_lagcov, L.sp_power_lagcov, L.sp_series_lagcov
        o = vp(out.ptr)
        assert ex(None, vp(d_in), data.size, width, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert ex(plan.h, vp(d_in), data.size, width, p(bands), 2, p(pairs), 2, lags, vp(out.ptr + 4)) == -1     # misaligned
        assert ex(plan.h, vp(d_in), data.size, width, p(bands), 2, p(pairs), 2, lags, None) == -1                # NULL
        assert ex(plan.h, vp(d_in), data.size, 0, p(bands), 2, p(pairs), 2, lags, None) == -1                    # ... at width 0 too: zeros are written
        assert ex(plan.h, vp(d_in), data.size, -1, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert ex(plan.h, None, data.size, width, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert ex(plan.h, vp(d_in), data.size, width, p(bands), 2, None, 2, lags, o) == -1                       # no pairs
        assert ex(plan.h, vp(d_in), data.size, width, None, 2, p(pairs), 2, lags, o) == -1                       # no bands
        assert ex(plan.h, vp(d_in), data.size, width, p(i32([0, n + 1, 3, 9])), 2, p(pairs), 2, lags, o) == -1   # what the band series refuses
        assert ex(plan.h, vp(d_in), data.size, width, p(i32([5, 4, 3, 9])), 2, p(pairs), 2, lags, o) == -1
        assert ex(plan.h, vp(d_in), data.size, width, p(bands), 65, p(pairs), 2, lags, o) == -1
        for bad in ([0, 2, 1, 1], [-1, 1, 1, 1], [0, 1, 1, 2]):                                                  # an index outside [0, count)
            assert ex(plan.h, vp(d_in), data.size, width, p(bands), 2, p(i32(bad)), 2, lags, o) == -1
        assert ex(plan.h, vp(d_in), data.size, width, p(bands), 0, p(pairs), 2, lags, o) == -1                   # ... [0, 0) holds none
        for npairs in (-1, 17):
            assert ex(plan.h, vp(d_in), data.size, width, p(bands), 2, p(i32([0, 1] * 17)), npairs, lags, o) == -1
        for bad in (0, -1, 1025):
            assert ex(plan.h, vp(d_in), data.size, width, p(bands), 2, p(pairs), 2, bad, o) == -1
        assert pw(None, vp(d_plane), n, width, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert pw(ctx.h, vp(d_plane), 0, width, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert pw(ctx.h, vp(d_plane), n, -1, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert pw(ctx.h, vp(d_plane + 4), n, width, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert pw(ctx.h, None, n, width, p(bands), 2, p(pairs), 2, lags, o) == -1
        assert pw(ctx.h, vp(d_plane), n, width, p(bands), 2, p(pairs), 2, lags, vp(out.ptr + 2)) == -1
        assert pw(ctx.h, vp(d_plane), n, width, p(bands), 2, p(i32([0, 2, 1, 1])), 2, lags, o) == -1
        assert pw(ctx.h, vp(d_plane), n, width, p(bands), 2, p(pairs), 2, 1025, o) == -1
        assert se(None, vp(d_plane), 2, width, p(pairs), 2, lags, o) == -1
        assert se(ctx.h, vp(d_plane), -1, width, p(pairs), 2, lags, o) == -1
        assert se(ctx.h, vp(d_plane), 65, width, p(pairs), 2, lags, o) == -1
        assert se(ctx.h, vp(d_plane), 2, -1, p(pairs), 2, lags, o) == -1
        assert se(ctx.h, vp(d_plane + 4), 2, width, p(pairs), 2, lags, o) == -1
        assert se(ctx.h, None, 2, width, p(pairs), 2, lags, o) == -1
        assert se(ctx.h, vp(d_plane), 2, width, None, 2, lags, o) == -1
        assert se(ctx.h, vp(d_plane), 2, width, p(pairs), 2, lags, None) == -1
        assert se(ctx.h, vp(d_plane), 2, width, p(pairs), 2, lags, vp(out.ptr + 4)) == -1
        assert se(ctx.h, vp(d_plane), 1, width, p(pairs), 2, lags, o) == -1                                      # index 1 of one series
        assert se(ctx.h, vp(d_plane), 2, width, p(pairs), 17, lags, o) == -1
        assert se(ctx.h, vp(d_plane), 2, width, p(pairs), 2, 0, o) == -1
        # requests that write nothing: no pair, or no band and no pair
        assert ex(plan.h, vp(d_in), data.size, width, p(bands), 2, None, 0, lags, None) == 0
        assert pw(ctx.h, vp(d_plane), n, width, None, 0, None, 0, lags, None) == 0
        assert se(ctx.h, None, 0, width, None, 0, lags, None) == 0
        assert L.sp_plan_lagcov_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
        assert (out.whole() == GARBAGE).all()
        assert pw(ctx.h, vp(d_plane), n, width, p(bands), 2, p(pairs), 2, lags, o) == 0      # ... and the same call with good arguments writes
        ctx.synchronize()
        assert (_bits(out.read("zeros")) == 0).all()
    finally:
        peak.close()
        plan.close()
        out.free()
        for p_ in (d_in, d_plane):
            ctx.free(p_)
    # the host entry
    rc, _, _, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, lags, detector="peak")
    assert rc == -4 and (host == GARBAGE).all()
    rc, _, _, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, -2, lags)
    assert rc == -1 and (host == GARBAGE).all()
    rc, _, _, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, lags, pairs=[(0, 4)])
    assert rc == -1 and (host == GARBAGE).all()
    rc, _, _, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, 1025)
    assert rc == -1 and (host == GARBAGE).all()
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "sample")
    res = np.full(3 * 2 * lags, 7.0)
    rl = L.sp_render_lagcov
    assert rl(None, C.byref(req), p(data), data.size, width, p(bands), 2, p(pairs), 2, lags, p(res)) == -1
    assert rl(ctx.h, None, p(data), data.size, width, p(bands), 2, p(pairs), 2, lags, p(res)) == -1
    assert rl(ctx.h, C.byref(req), None, data.size, width, p(bands), 2, p(pairs), 2, lags, p(res)) == -1
    assert rl(ctx.h, C.byref(req), p(data), data.size, width, p(bands), 2, p(pairs), 2, lags, None) == -1
    assert rl(ctx.h, C.byref(req), p(data), data.size, width, p(bands), 2, p(pairs), 2, lags, vp(res.ctypes.data + 4)) == -1
    assert (res == 7.0).all()
    rc, got, intact, _ = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, lags)
    assert rc == 0 and intact and np.isfinite(got).all() and (got[0] > 0).all() and (got[2] > 0).all() and got[1].any()


def _own_cu_count(ctx):
    """The part's own CU count, as sp_plan_debug_launch reports it on a context without an override."""
    win, weight = pyoracle.window("hann", 64)
    plan = ctx.plan("CU8", 64, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        return plan.debug_launch(2 * 64 * 4, 4)["cu_count"]
    finally:
        plan.close()


def test_the_cu_count_does_not_change_a_bit(pkg, ctx):
    """At 1 CU the 1031 terms of 3 pairs of 33 lags (6 bands) stay in one piece, at the part's own count they are cut into 33.
    sp_context_debug_set_cu_count admits 1 ... the part's own count: where it refuses 304, the launch rule itself
    (sp_debug_lagcov_launch, the function the launch calls) must give this request at 304 CUs the very grid it gets at the part's own
    count, and that launch is the one compared."""
    lags, terms = 33, 1031
    series, want = _sweep(lags, terms)
    b = pkg.binding
    own = _own_cu_count(ctx)
    base = _series_lagcov(ctx, series, SWEEP_PAIRS, lags, "own count")
    lagcovref.assert_same(base, want, "own count")
    assert b.debug_lagcov_launch(3, lags, terms, 1) == (6, 1, 1031) and b.debug_lagcov_launch(3, lags, terms, own)[1] == 33
    try:
        for cu in (1, 304):
            try:
                ctx.set_cu_count(cu)
            except pkg.SpectroplotError:
                ctx.set_cu_count(0)
                assert own < cu and b.debug_lagcov_launch(3, lags, terms, cu) == b.debug_lagcov_launch(3, lags, terms, own)
            got = _series_lagcov(ctx, series, SWEEP_PAIRS, lags, "cu %d" % cu)
            assert np.array_equal(_bits(got), _bits(base)), cu
            lagcovref.assert_same(got, want, "cu %d" % cu)
    finally:
        ctx.set_cu_count(0)
