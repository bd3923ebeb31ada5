"""The exact variance and spectral-kurtosis traces on the GPU (sp_power_variance, sp_plan_execute_variance, sp_render_variance): every
comparison is bit for bit against tests/varianceref.py - exact rational sums, squares and their difference, rounded once - on a synthetic
plane or on the oracle's plane (tests/powerref.py, the references of tests/test_mean_gpu.py shared); which NaN a NaN is, is the one
thing left uncompared.  Every result lies between guard bytes and holds garbage before the call.

There is no n = 2^20 case: rows are independent, and n enters only the grid's x and the workspace's stride, which n = 2048 and n = 100
cover; its 1.7 GB workspace and its rational reference do not fit a test of a few seconds.  The measurement that
goes with the feature is not asserted here (tools/variance_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import meanref
import powerref
import siggen
import varianceref
from __graft_entry__ import load_package
from oracle import pyoracle
from test_gpu_parity import _assert_same as assert_same_reply
from test_mean_gpu import GARBAGE, GEN, GUARD, _capture, _power_mean, _reference, _upload

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
    """A device array f64 [3, n] between two guards, everything garbage."""

    def __init__(self, ctx, n):
        self.ctx, self.n, self.bytes = ctx, n, 24 * n
        self.base = ctx.alloc(self.bytes + 2 * GUARD)
        assert self.base % 8 == 0
        self.ptr = self.base + GUARD
        ctx.memset(self.base, GARBAGE, self.bytes + 2 * GUARD)

    def whole(self):
        return self.ctx.download(self.base, self.bytes + 2 * GUARD)

    def read(self, what=""):
        whole = self.whole()
        assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + self.bytes:] == GARBAGE).all(), what + ": bytes around the reply were written"
        return whole[GUARD:GUARD + self.bytes].view(np.float64).reshape(3, self.n).copy()

    def free(self):
        self.ctx.free(self.base)


def _power_variance(ctx, plane, what):
    """sp_power_variance of a host plane f64 [width, n] through a device copy."""
    width, n = plane.shape
    d_p, out = _upload(ctx, plane), _Out(ctx, n)
    try:
        ctx.power_variance(d_p if width else 0, n, width, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_p)
        out.free()


def _execute_variance(ctx, plan, d_in, nbytes, width, n, what):
    out = _Out(ctx, n)
    try:
        plan.execute_variance(d_in, nbytes, width, out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- (a) sp_power_variance on synthetic planes ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(n, width):
    plane = varianceref.synthetic_plane(3000 * n + width, width, n)
    plane.setflags(write=False)
    want = varianceref.expected(plane)
    want.setflags(write=False)
    return plane, want


@pytest.mark.parametrize("width", [1, 2, 3, 17, 33, 257])
@pytest.mark.parametrize("n", [2, 32, 64, 100, 256])
def test_power_variance_of_synthetic_planes(ctx, n, width):
    """The full exponent range, denormals, cell-boundary exponents and a frame of DBL_MAX, constant rows, one-ulp rows and rows with a
    NaN, a +inf and both.  n: below, at half of, at, off a multiple of and several times 64 rows (the workgroup's band is 32); W: below
    and past the frames a workgroup has in flight, and past one and several 32-frame pieces.  out[0] / W is sp_power_mean's trace."""
    plane, want = _synthetic(n, width)
    what = "sp_power_variance n=%d W=%d" % (n, width)
    got = _power_variance(ctx, plane, what)
    varianceref.assert_same(got, want, what)
    with np.errstate(all="ignore"):
        meanref.assert_same(got[0] / np.float64(width), _power_mean(ctx, plane, what), what + ": out[0] / W against sp_power_mean")
    if n >= 16:
        assert _bits(got)[2, 7] == 0 and np.isfinite(got[:, 7]).all()                       # the constant row: +0.0 exactly
        assert np.isnan(got[:, 13]).all() and np.isinf(got[:, 14]).all()
        assert np.isnan(got[:, 15]).all() if width > 1 else True
        assert got[0, 9] == np.finfo(np.float64).max if width == 1 else np.isinf(got[1, 9])  # DBL_MAX in one frame: its square is +inf
        if width > 1:
            assert 0 < got[2, 8] < 1e-30 and np.isfinite(got[:, 8]).all()                   # one ulp in one frame: tiny, positive, exact
            p = plane[:, 8]
            naive = width * np.sum(p * p) - np.sum(p) ** 2
            assert naive != got[2, 8]                                                        # ... where the f64 form has only noise


def test_power_variance_nan_and_inf_rule(ctx):
    n, width = 64, 257
    plane = _synthetic(n, width)[0].copy()
    plane[100, 1] = np.nan            # a NaN in one frame of one row
    plane[3, 2] = np.inf              # an inf in another
    plane[200, 3] = np.inf
    plane[201, 3] = np.nan            # NaN beats inf
    plane[256, 4] = np.inf            # the last frame
    plane[0, 63] = np.nan             # the first frame of the last row
    want = varianceref.expected(plane)
    assert np.isnan(want[:, 1]).all() and np.isinf(want[:, 2]).all() and np.isnan(want[:, 3]).all() and np.isinf(want[:, 4]).all()
    assert np.isnan(want[:, 63]).all() and np.isfinite(want[:, 7]).all()
    varianceref.assert_same(_power_variance(ctx, plane, "specials"), want, "sp_power_variance specials")


@pytest.mark.parametrize("n", [2, 64, 256])
def test_power_variance_of_no_frames_is_zero(ctx, n):
    got = _power_variance(ctx, np.zeros((0, n)), "width 0")
    assert got.shape == (3, n) and (_bits(got) == 0).all()


def _own_cu_count(ctx):
    """The part's own CU count, as sp_plan_debug_launch reports it on a context without an override."""
    win, weight = pyoracle.window("hann", 64)
    plan = ctx.plan("CU8", 64, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        return plan.debug_launch(2 * 64 * 4, 4)["cu_count"]
    finally:
        plan.close()


def test_the_cu_count_does_not_change_a_bit(pkg, ctx):
    """At 1 CU the frames of n = 100, W = 257 are cut into 2 pieces, at the part's own count into 9.  sp_context_debug_set_cu_count
    admits 1 ... the part's own count: where it refuses 304, the launch rule itself (sp_debug_variance_launch, the function the launch
    calls) must give this plane at 304 CUs the very grid it gets at the part's own count, and that launch is the one compared."""
    n, width = 100, 257
    plane, want = _synthetic(n, width)
    b = pkg.binding
    own = _own_cu_count(ctx)
    base = _power_variance(ctx, plane, "own count")
    varianceref.assert_same(base, want, "own count")
    assert b.debug_variance_launch(n, width, 1) == (4, 2, 129) and b.debug_variance_launch(n, width, own)[1] == 9
    try:
        for cu in (1, 304):
            try:
                ctx.set_cu_count(cu)
            except pkg.SpectroplotError:
                ctx.set_cu_count(0)
                assert own < cu and b.debug_variance_launch(n, width, cu) == b.debug_variance_launch(n, width, own)
            got = _power_variance(ctx, plane, "cu %d" % cu)
            assert np.array_equal(_bits(got)[~np.isnan(got)], _bits(base)[~np.isnan(base)]), cu
            varianceref.assert_same(got, want, "cu %d" % cu)
    finally:
        ctx.set_cu_count(0)


# ---- (b) sp_plan_execute_variance against the oracle's plane: the window, the interleaving ------------------------------------------------
ORACLE = [("CF32", 64, 37, "frames_power"), ("CS16", 1024, 37, "frames_power"), ("CF32", 2048, 2, "scratch_power")]


@functools.lru_cache(maxsize=None)
def _want(fmt, n, width, stride):
    """The variance sums of the plane test_mean_gpu's reference holds for this request."""
    want = varianceref.expected(_reference(fmt, n, width, False, stride)[3])
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("fmt,n,width,name", ORACLE, ids=["n%d" % c[1] for c in ORACLE])
def test_execute_variance_against_the_oracle_whatever_the_window(ctx, fmt, n, width, name):
    data, win, bn, plane, mean = _reference(fmt, n, width, False, n // 2 + 3)
    want = _want(fmt, n, width, n // 2 + 3)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, data)
    got = []
    try:
        assert plan.variance_kernel_name_for(data.size, width) == name + "+variance"
        for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, below one frame (one frame), the default
            ctx.set_mean_window(window)
            got.append(_execute_variance(ctx, plan, d_in, data.size, width, n, "window %d" % window))
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()
    for g in got:
        varianceref.assert_same(g, want, "%s n=%d W=%d" % (fmt, n, width))
        assert np.array_equal(_bits(g), _bits(got[0]))
    s1, s2, d = got[0]
    assert np.array_equal(_bits(s1 / np.float64(width)), _bits(mean))          # the mean's trace, bit for bit
    assert (s1 > 0).all() and (s2 > 0).all() and (d >= 0).all() and (d > 0).sum() > n // 2 and (d < width * s2).all()


def test_execute_variance_interleaves_without_a_synchronisation(ctx):
    fmt, n, width = "CS16", 1024, 37
    data, win, bn, _, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want = _want(fmt, n, width, n // 2 + 3)
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
        plan.execute_variance(d_in, data.size, width, out.ptr)
        plan.execute(d_in, data.size, width, *second)
        ctx.synchronize()
        assert_same_reply(reply(first), r_want)
        assert_same_reply(reply(second), r_want)
        varianceref.assert_same(out.read("interleaved"), want, "interleaved")
    finally:
        out.free()
        for p_ in first + second + [d_in]:
            ctx.free(p_)
        plan.close()


# ---- (c) the host entry point -------------------------------------------------------------------------------------------------------------------
def _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, detector="sample"):
    """sp_render_variance into a host array between guards, everything garbage: (status, the reply, nothing but it was written, the
    whole array)."""
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, False, False, detector)
    size = 24 * n
    host = np.full(size + 2 * GUARD, GARBAGE, np.uint8)
    vp = C.c_void_p
    rc = ctx.lib.L.sp_render_variance(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, width, vp(host.ctypes.data + GUARD))
    intact = bool((host[:GUARD] == GARBAGE).all() and (host[GUARD + size:] == GARBAGE).all())
    return rc, host[GUARD:GUARD + size].view(np.float64).reshape(3, n).copy(), intact, host


def test_dense_render_variance(pkg, ctx):
    fmt, n, width = "CF32", 64, 37
    data, win, bn, _, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want = _want(fmt, n, width, n // 2 + 3)
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width)
    assert rc == 0 and intact
    varianceref.assert_same(got, want, "dense sp_render_variance")
    varianceref.assert_same(ctx.render_variance(fmt, data, n, win, bn, 3.0, 50.0, width, fill=GARBAGE), want, "Context.render_variance")


def test_small_sparse_request_uploads_its_frames_only(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, _ = _reference(fmt, n, width, False, 40 * n + 11)
    want = _want(fmt, n, width, 40 * n + 11)
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width)
    assert rc == 0 and intact
    varianceref.assert_same(got, want, "sparse sp_render_variance")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1


def test_chunked_sp_render_variance(pkg, ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts: the capture travels in chunks and the cells accumulate over them."""
    fmt, n, width = "CF32", 1024, 2048
    data, win, bn, _, _ = _reference(fmt, n, width, False, n)
    want = _want(fmt, n, width, n)
    assert data.size >= 16 << 20
    rc, got, intact, _ = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width)
    assert rc == 0 and intact
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    varianceref.assert_same(got, want, "chunked sp_render_variance")


# ---- (d) no frames, and refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 2048])
def test_a_capture_shorter_than_n_and_a_request_of_no_frames(pkg, ctx, n):
    """A capture shorter than n: the oracle's plane is NaN in every frame, so the mean's rule gives NaN in all three arrays.  W = 0, of
    that capture and of a long one: 3 n times +0.0, the sums of nothing."""
    data = siggen.generate("CS16", GEN, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    plane = powerref.expected("CS16", data, n, win, 1.0 / weight, 3.0, 50.0, 3, False)["power"]
    want = varianceref.expected(plane)
    assert plane.shape == (3, n) and np.isnan(want).all()
    rc, got, intact, _ = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, 3)
    assert rc == 0 and intact
    varianceref.assert_same(got, want, "a capture shorter than n")
    rc, got, intact, _ = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, 0)
    assert rc == 0 and intact and (_bits(got) == 0).all()
    long = _capture("CS16", n, 4, n)
    plan = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, long)
    try:
        got = _execute_variance(ctx, plan, d_in, long.size, 0, n, "W = 0")
        assert (_bits(got) == 0).all()
    finally:
        ctx.free(d_in)
        plan.close()


def test_refusals_write_nothing(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    vp = C.c_void_p
    d_in, d_plane, out = _upload(ctx, data), ctx.alloc(8 * width * n + 16), _Out(ctx, n)
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        ctx.memset(d_plane, 0, 8 * width * n + 16)
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_variance(d_in, data.size, width, out.ptr)
        assert e.value.status == -4 and "peak" in str(e.value)
        ex, pv = L.sp_plan_execute_variance, L.sp_power_variance
        assert ex(None, vp(d_in), data.size, width, vp(out.ptr)) == -1
        assert ex(plan.h, vp(d_in), data.size, width, vp(out.ptr + 4)) == -1       # misaligned
        assert ex(plan.h, vp(d_in), data.size, width, None) == -1                  # NULL
        assert ex(plan.h, vp(d_in), data.size, 0, None) == -1                      # ... at width 0 too: 3 n zeros are written
        assert ex(plan.h, vp(d_in), data.size, -1, vp(out.ptr)) == -1
        assert ex(plan.h, None, data.size, width, vp(out.ptr)) == -1
        assert pv(None, vp(d_plane), n, width, vp(out.ptr)) == -1
        assert pv(ctx.h, vp(d_plane), 0, width, vp(out.ptr)) == -1
        assert pv(ctx.h, vp(d_plane), (1 << 20) + 1, width, vp(out.ptr)) == -1     # n beyond SP_MAX_N
        assert pv(ctx.h, vp(d_plane), n, -1, vp(out.ptr)) == -1
        assert pv(ctx.h, vp(d_plane + 4), n, width, vp(out.ptr)) == -1
        assert pv(ctx.h, vp(d_plane), n, width, vp(out.ptr + 2)) == -1
        assert pv(ctx.h, vp(d_plane), n, width, None) == -1
        assert pv(ctx.h, None, n, width, vp(out.ptr)) == -1
        assert L.sp_plan_variance_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
        assert (out.whole() == GARBAGE).all()
        assert pv(ctx.h, vp(d_plane), n, width, vp(out.ptr)) == 0                  # ... and the same call with good arguments writes
        ctx.synchronize()
        assert (_bits(out.read("zeros")) == 0).all()
    finally:
        peak.close()
        plan.close()
        out.free()
        for p_ in (d_in, d_plane):
            ctx.free(p_)
    # the host entry
    rc, _, _, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width, detector="peak")
    assert rc == -4 and (host == GARBAGE).all()
    rc, _, _, host = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, -2)
    assert rc == -1 and (host == GARBAGE).all()
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "sample")
    res = np.full(3 * n, 7.0)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    rv = L.sp_render_variance
    assert rv(None, C.byref(req), p(data), data.size, width, p(res)) == -1
    assert rv(ctx.h, None, p(data), data.size, width, p(res)) == -1
    assert rv(ctx.h, C.byref(req), None, data.size, width, p(res)) == -1
    assert rv(ctx.h, C.byref(req), p(data), data.size, width, None) == -1
    assert rv(ctx.h, C.byref(req), p(data), data.size, width, vp(res.ctypes.data + 4)) == -1
    assert (res == 7.0).all()
    rc, got, intact, _ = _render_guarded(ctx, pkg, "CU8", data, n, win, 1.0 / weight, width)
    assert rc == 0 and intact and np.isfinite(got).all() and (got[:2] > 0).all() and (got[2] >= 0).all() and got[2].any()
