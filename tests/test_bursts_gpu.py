"""The burst lists on the GPU (sp_series_bursts, sp_power_bursts, sp_plan_execute_bursts, sp_render_bursts): every comparison is of whole
integer arrays for equality against tests/burstref.py - a plain loop of floating-point compares - on burstref's planted series, on
bandref's exact band sums of a synthetic plane, or on those of the oracle's plane (tests/powerref.py).  Every result lies between guard
bytes and holds garbage before the call.  There is no tolerance anywhere.

The measurement that goes with the feature is not asserted here (tools/burst_bench.py)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bandref
import burstref
import meanref
import powerref
import quantileref
from __graft_entry__ import ROOT, load_package
from oracle import pyoracle
from test_density_gpu import _hip_runtime
from test_mean_gpu import FORMATS, GARBAGE, GUARD, KERNELS, _capture, _Out, _reference, _upload
from test_track_gpu import _hop_reference

pytestmark = pytest.mark.gpu

_HDR = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
S = int(re.search(r"^#define SP_BURST_SEGMENT_FRAMES (\d+)$", _HDR, re.M).group(1))
WIDTHS_A = (1, 2, 63, 64, 65, 257, S - 1, S, S + 1, 2 * S + 3, 64 * S + 5)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Words:
    """The two device outputs, counts uint32 [count] and edges int32 [count, m, 2], each between two guards, everything garbage."""

    def __init__(self, ctx, count, m, counts=True, edges=True):
        self.ctx, self.count, self.m = ctx, count, m
        self.sizes = (4 * count if counts else 0, 8 * count * m if edges else 0)
        self.base = [ctx.alloc(s + 2 * GUARD) for s in self.sizes]
        for b, s in zip(self.base, self.sizes):
            ctx.memset(b, GARBAGE, s + 2 * GUARD)
        self.counts = self.base[0] + GUARD if counts else 0
        self.edges = self.base[1] + GUARD if edges and m > 0 else 0

    def read(self, what=""):
        """(counts or None, edges or None)"""
        out = []
        for b, s, present in zip(self.base, self.sizes, (self.counts, self.edges)):
            whole = self.ctx.download(b, s + 2 * GUARD)
            assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + s:] == GARBAGE).all(), what + ": bytes around an output were written"
            out.append(whole[GUARD:GUARD + s].copy() if present else None)
        counts = out[0].view(np.uint32) if out[0] is not None else None
        edges = out[1].view(np.int32).reshape(self.count, self.m, 2) if out[1] is not None else None
        return counts, edges

    def free(self):
        for b in self.base:
            self.ctx.free(b)


def assert_same(got, want, what):
    """Whole arrays for equality; a None on the left is an output that was not asked for."""
    for g, w, name in zip(got, want, ("counts", "edges")):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %r %r, want %r %r" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            at = tuple(np.argwhere(g != w)[0])
            raise AssertionError("%s: the %s differ in %d of %d words, first at %r: got %r, want %r"
                                 % (what, name, int((g != w).sum()), w.size, at, g[at], w[at]))


def _series_bursts(ctx, d_series, count, width, hi, lo, m, what, counts=True, edges=True):
    out = _Words(ctx, count, m, counts, edges)
    try:
        ctx.series_bursts(d_series if count * width else 0, count, width, hi, lo, m, out.counts, out.edges)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


# ---- (a) sp_series_bursts on planted series ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS_A, ids=["W%d" % w for w in WIDTHS_A])
def test_series_bursts_of_planted_series(ctx, width):
    """count 1, 3 and 64; max_bursts 0 (counts only), 1, 7 and width // 2 + 1 (nothing is cut); both outputs, and each alone.  The
    widths lie around the 64 frames of a load and around the segment; 64 S + 5 makes the carry scan take a second step of 64
    summaries.  What the series holds is asserted on the reference's output (burstref.telling); a slot behind a band's count is -1
    in the reference, so equality checks it."""
    for seed in (0, 1) if width <= 257 else (0,):
        for count in (1, 3, 64):
            series, hi, lo = burstref.planted_series(seed, count, width, S)
            need = burstref.must_tell(seed, count, width, S)
            assert need <= burstref.telling(series, hi, lo, S), (seed, count, width)
            full = burstref.planted_expected(seed, count, width, S)
            assert (full[1][np.arange(width // 2 + 1)[None, :] >= full[0][:, None]] == -1).all()
            d_series = _upload(ctx, series)
            try:
                for m in (0, 1, 7, width // 2 + 1):
                    want = burstref.cut(*full, m)
                    what = "sp_series_bursts seed %d count %d W=%d max_bursts %d" % (seed, count, width, m)
                    assert_same(_series_bursts(ctx, d_series, count, width, hi, lo, m, what), want, what)
                    if m in (0, 7):
                        got = _series_bursts(ctx, d_series, count, width, hi, lo, m, what, edges=False)
                        assert got[1] is None
                        assert_same(got, want, what + " counts alone")
                    if m == 7:
                        got = _series_bursts(ctx, d_series, count, width, hi, lo, m, what, counts=False)
                        assert got[0] is None
                        assert_same(got, want, what + " edges alone")
            finally:
                ctx.free(d_series)


def test_series_bursts_reads_values_by_key(ctx):
    """The sign bit of a value is not looked at: the negated series gives the same words."""
    series, hi, lo = burstref.planted_series(0, 6, 300, S)
    want = burstref.cut(*burstref.planted_expected(0, 6, 300, S), 9)
    d = _upload(ctx, -series)
    try:
        assert_same(_series_bursts(ctx, d, 6, 300, hi, lo, 9, "negated"), want, "negated")
    finally:
        ctx.free(d)


# ---- (b) sp_power_bursts on a synthetic plane --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gated_plane(n, width):
    """A plane f64 [width, n] whose rows are keyed on and off in runs of frames, its bands (overlapping, empty, single-row), their exact
    sums by bandref and thresholds of three quarters and one quarter of every band's strongest sum."""
    rng = np.random.default_rng(77 * n + width)
    gate = np.repeat(rng.random((width + 6) // 7 + 1) < 0.4, 7)[:width]
    plane = rng.uniform(0.5, 1.5, (width, n)) * np.where(gate, 100.0, 1.0)[:, None]
    plane[rng.random((width, n)) < 0.01] = 0.0
    bands = bandref.standard_bands(n)
    sums = bandref.expected(plane, bands)
    top = sums.max(axis=1)
    hi, lo = 0.75 * top, 0.25 * top                 # (the empty band: 0 and 0, every frame a SET)
    for a in (plane, sums, hi, lo):
        a.setflags(write=False)
    return plane, bands, sums, hi, lo


@pytest.mark.parametrize("n,width", [(2, 300), (100, S + 1), (256, 300)])
def test_power_bursts_of_a_synthetic_plane(ctx, n, width):
    """sp_power_bursts == sp_series_bursts of sp_power_bands of the same plane == burstref of bandref's exact sums."""
    plane, bands, sums, hi, lo = _gated_plane(n, width)
    m = 16
    want = burstref.expected(sums, hi, lo, m)
    assert (want[0] > 2).sum() >= 3 and (want[0][0] == 1) and (want[1][0, 0] == (0, width)).all()     # bursts, and the empty band's one
    assert (want[0] > m).any() or width < 1000
    count = len(bands)
    d_p, d_s = _upload(ctx, plane), ctx.alloc(8 * count * width)
    direct, chained = _Words(ctx, count, m), _Words(ctx, count, m)
    try:
        ctx.power_bursts(d_p, n, width, bands, hi, lo, m, direct.counts, direct.edges)
        ctx.power_bands(d_p, n, width, bands, d_s)
        ctx.series_bursts(d_s, count, width, hi, lo, m, chained.counts, chained.edges)
        ctx.synchronize()
        got_sums = ctx.download(d_s, 8 * count * width, np.float64).reshape(count, width)
        bandref.assert_same(got_sums, sums, "sp_power_bands")
        assert_same(direct.read("direct"), want, "sp_power_bursts n=%d W=%d" % (n, width))
        assert_same(chained.read("chained"), want, "sp_series_bursts of sp_power_bands")
    finally:
        for o in (direct, chained):
            o.free()
        for p_ in (d_p, d_s):
            ctx.free(p_)


# ---- (c) sp_plan_execute_bursts against the oracle's plane ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_reference(fmt, n, width, ch, m=12):
    """(capture, taper, block_norm, bands, hi, lo, expected) on test_track_gpu's hopping capture: the thresholds are every band
    series' own median times 4 and times 2."""
    data, win, bn, plane, _ = _hop_reference(fmt, n, width, ch, n // 2 + 3)
    bands = bandref.standard_bands(n)
    sums = bandref.expected(plane, bands)
    median = np.sort(sums, axis=1)[:, (width - 1) // 2]
    hi, lo = 4.0 * median, 2.0 * median
    want = burstref.expected(sums, hi, lo, m)
    for a in (hi, lo) + want:
        a.setflags(write=False)
    return data, win, bn, bands, hi, lo, want


def _execute_bursts(ctx, plan, d_in, nbytes, width, bands, hi, lo, m, what):
    out = _Words(ctx, len(bands), m)
    try:
        plan.execute_bursts(d_in, nbytes, width, bands, hi, lo, m, out.counts, out.edges)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


ORACLE_WIDTHS = (2, 37)


@pytest.mark.parametrize("k", range(len(KERNELS)), ids=["n%d%s" % (n, "-forced" if f else "") for n, f, _ in KERNELS])
@pytest.mark.parametrize("width", ORACLE_WIDTHS, ids=["W%d" % w for w in ORACLE_WIDTHS])
def test_execute_bursts_against_the_oracle(ctx, k, width):
    """Every (kernel, n) of the mean's oracle test; the format and the channel mode rotate as there."""
    n, forced, name = KERNELS[k]
    j = ORACLE_WIDTHS.index(width)
    fmt, ch = FORMATS[(k + j) % 3], (k // 3 + j) % 2 == 1
    data, win, bn, bands, hi, lo, want = _oracle_reference(fmt, n, width, ch)
    what = "%s n=%d W=%d%s%s" % (fmt, n, width, " L/R" if ch else "", " forced" if forced else "")
    if width >= 37:   # on the reference: a band with a burst, and one with a fall
        assert (want[0] > 0).any() and ((want[1][:, :, 1] >= 0) & (want[1][:, :, 1] < width)).any(), what
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.bursts_kernel_name_for(data.size, width) == name + "+bursts"
        assert_same(_execute_bursts(ctx, plan, d_in, data.size, width, bands, hi, lo, 12, what), want, what)
    finally:
        ctx.free(d_in)
        plan.close()


# ---- (d) independence of the window, the chunking and the layout -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 256, 300, False), ("CF32", 1024, 37, True)])
def test_the_window_and_the_layout_do_not_change_a_word(ctx, fmt, n, width, ch):
    data, win, bn, bands, hi, lo, want = _oracle_reference(fmt, n, width, ch)
    assert (want[0] > 0).any()
    d_in = _upload(ctx, data)
    got = []
    try:
        for waterfall in (False, True):
            plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch, waterfall)
            try:
                for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, one byte (one frame), the default
                    ctx.set_mean_window(window)
                    got.append(_execute_bursts(ctx, plan, d_in, data.size, width, bands, hi, lo, 12, "window %d" % window))
            finally:
                ctx.set_mean_window(0)
                plan.close()
    finally:
        ctx.free(d_in)
    for g in got:
        assert_same(g, want, "window / layout")


def test_chunked_sp_render_bursts_whose_chunks_cut_a_burst(ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts, on multiples of 32 frames: a burst that runs over all frames (the
    band of every row against hi = 0) and the median's bursts of the other bands, with the default window and with one of five frames."""
    fmt, n, width = "CF32", 1024, 2048
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n)
    assert data.size >= 16 << 20
    bands = [(0, n), (0, 1), (n // 4, n // 2), (5, 5)]
    sums = _band_sums(fmt, n, width, tuple(bands))
    median = np.sort(sums, axis=1)[:, (width - 1) // 2]
    hi, lo = 1.25 * median, 0.8 * median
    hi[0] = lo[0] = 0.0
    want = burstref.expected(sums, hi, lo, 40)
    assert want[0][0] == 1 and (want[1][0, 0] == (0, width)).all()
    crossing = [(s, e) for s, e in want[1][1:].reshape(-1, 2) if s >= 0 and s // 32 != (e - 1) // 32]
    assert crossing, "no burst of the reference crosses a multiple of 32 frames"
    try:
        ctx.set_mean_window(5 * 8 * n)
        got = ctx.render_bursts(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, 40, fill=GARBAGE)
        assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    finally:
        ctx.set_mean_window(0)
    assert_same(got, want, "a window of five frames")
    default = ctx.render_bursts(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, 40, fill=GARBAGE)
    assert ctx.last_chunks() > 1
    assert_same(default, want, "the default window")
    waterfall = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, False, True)
    d_in = _upload(ctx, data)
    try:
        assert_same(_execute_bursts(ctx, waterfall, d_in, data.size, width, bands, hi, lo, 40, "resident"), want, "the capture resident")
    finally:
        ctx.free(d_in)
        waterfall.close()


@functools.lru_cache(maxsize=None)
def _band_sums(fmt, n, width, bands):
    return bandref.expected(_reference(fmt, n, width, False, n)[3], list(bands))


def test_small_sparse_request_and_scalar_thresholds(pkg, ctx):
    """sp_render_bursts into host arrays between guards; a number for hi and lo is every band's."""
    fmt, n, width = "CU8", 256, 64
    data, win, bn, plane, _ = _hop_reference(fmt, n, width, False, 40 * n + 11)
    bands = bandref.standard_bands(n)
    sums = bandref.expected(plane, bands)
    hi = float(np.median(sums[1]) * 4.0)               # (four times the median of the single row's series)
    lo = hi / 4
    m = 5
    want = burstref.expected(sums, [hi] * len(bands), [lo] * len(bands), m)
    assert want[0][1] >= 2 and want[0][0] == 0
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, False, False)
    b = np.ascontiguousarray(bands, np.int32)
    h, l = np.full(len(bands), hi), np.full(len(bands), lo)
    sizes = (4 * len(bands), 8 * len(bands) * m)
    host = [np.full(s + 2 * GUARD, GARBAGE, np.uint8) for s in sizes]
    vp = C.c_void_p
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    rc = ctx.lib.L.sp_render_bursts(ctx.h, C.byref(req), p(data), data.size, width, p(b), len(bands), p(h), p(l), m,
                                    vp(host[0].ctypes.data + GUARD), vp(host[1].ctypes.data + GUARD))
    assert rc == 0
    for a, s in zip(host, sizes):
        assert (a[:GUARD] == GARBAGE).all() and (a[GUARD + s:] == GARBAGE).all()
    got = (host[0][GUARD:GUARD + sizes[0]].view(np.uint32), host[1][GUARD:GUARD + sizes[1]].view(np.int32).reshape(len(bands), m, 2))
    assert_same(got, want, "sparse sp_render_bursts")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1
    assert_same(ctx.render_bursts(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, m, fill=GARBAGE), want, "scalar thresholds")
    widths, gaps = pkg.burst_pulses(got[1][1], got[0][1])
    assert (widths > 0).all() and (gaps > 0).all() and len(widths) == min(int(got[0][1]), m) and len(gaps) == len(widths) - 1


# ---- (e) no frames, no bands, refusals ---------------------------------------------------------------------------------------------------------
def test_width_0_and_count_0(pkg, ctx):
    n = 128
    data = _capture("CU8", n, 20, 3 * n)
    win, weight = pyoracle.window("hann", n)
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, data)
    bands = [(0, n), (3, 9), (0, 0)]
    try:
        for m in (0, 4):
            out = _Words(ctx, 3, m)
            plan.execute_bursts(d_in, data.size, 0, bands, 2.0, 1.0, m, out.counts, out.edges)          # width == 0
            ctx.synchronize()
            counts, edges = out.read("width 0")
            assert counts.tolist() == [0, 0, 0] and (edges is None or (edges == -1).all())
            out.free()
        out = _Words(ctx, 3, 4)
        ctx.power_bursts(0, n, 0, bands, 2.0, 1.0, 4, out.counts, out.edges)
        ctx.series_bursts(0, 3, 0, 2.0, 1.0, 4, out.counts, 0)
        ctx.synchronize()
        counts, edges = out.read("width 0, resident")
        assert counts.tolist() == [0, 0, 0] and (edges == -1).all()
        out.free()
        out = _Words(ctx, 3, 4)                                                                        # count == 0: nothing is written
        plan.execute_bursts(d_in, data.size, 20, [], 2.0, 1.0, 4, out.counts, out.edges)
        ctx.series_bursts(d_in, 0, 20, 2.0, 1.0, 4, out.counts, out.edges)
        ctx.synchronize()
        counts, edges = out.read("count 0")
        assert (counts.view(np.uint8) == GARBAGE).all() and (edges.view(np.uint8) == GARBAGE).all()
        out.free()
    finally:
        ctx.free(d_in)
        plan.close()
    counts, edges = ctx.render_bursts("CU8", data, n, win, 1.0 / weight, 3.0, 50.0, 0, bands, 2.0, 1.0, 4, fill=GARBAGE)
    assert counts.tolist() == [0, 0, 0] and edges.shape == (3, 4, 2) and (edges == -1).all()
    counts, edges = ctx.render_bursts("CU8", data, n, win, 1.0 / weight, 3.0, 50.0, 20, [], 2.0, 1.0, 4, fill=GARBAGE)
    assert counts.size == 0 and edges.size == 0


def test_refusals(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    d_in, d_plane = ctx.alloc(data.size), ctx.alloc(8 * width * n + 16)
    out = _Words(ctx, 4, 4)
    vp = C.c_void_p
    nan = float("nan")

    def ints(*v):
        return (C.c_int32 * len(v))(*v)

    def dbl(*v):
        return (C.c_double * len(v))(*v)

    ok_b, ok_h, ok_l = ints(0, n, 3, 9), dbl(4.0, 4.0), dbl(1.0, 4.0)
    # (bands, count, hi, lo, max_bursts, counts, edges)
    good = (ok_b, 2, ok_h, ok_l, 4, vp(out.counts), vp(out.edges))
    bad = [(ints(0, n + 1, 3, 9),) + good[1:], (ints(5, 4, 3, 9),) + good[1:], (ints(-1, 4, 3, 9),) + good[1:],          # bad bands
           (None,) + good[1:], (ok_b, -1) + good[2:], (ints(*([0, 1] * 65)), 65, dbl(*([4.0] * 65)), dbl(*([1.0] * 65))) + good[4:],
           good[:2] + (dbl(4.0, nan),) + good[3:], good[:3] + (dbl(nan, 1.0),) + good[4:],                              # a NaN threshold
           good[:3] + (dbl(1.0, 4.5),) + good[4:], good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:],         # lo > hi; none
           good[:4] + (-1,) + good[5:], good[:4] + (2 ** 29,) + good[5:],                                               # max_bursts
           good[:5] + (None, None), good[:4] + (0, None, vp(out.edges)),                                               # both outputs absent
           good[:5] + (vp(out.counts + 2), vp(out.edges)), good[:5] + (vp(out.counts), vp(out.edges + 1))]              # misaligned
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "peak")
    host_c, host_e = np.full(4, 7, np.uint32), np.full(32, 7, np.int32)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_bursts(d_in, data.size, width, [(0, n)], 4.0, 1.0, 4, out.counts, out.edges)
        assert e.value.status == -4 and "peak" in str(e.value)
        ex, pw, se, rt = L.sp_plan_execute_bursts, L.sp_power_bursts, L.sp_series_bursts, L.sp_render_bursts
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok_b, 2, ok_h, ok_l, 4, p(host_c), p(host_e)) == -4
        req.detector = 0
        assert ex(None, vp(d_in), data.size, width, *good) == -1
        for k, args in enumerate(bad):
            assert ex(plan.h, vp(d_in), data.size, width, *args) == -1, k
            assert pw(ctx.h, vp(d_plane), n, width, *args) == -1, k
            host = args[:5] + tuple(a if a is None else p(h) for a, h in zip(args[5:], (host_c, host_e)))
            if k < len(bad) - 2:
                assert rt(ctx.h, C.byref(req), p(data), data.size, width, *host) == -1, k
            if k >= 4:                                                       # (the series has no bands)
                assert se(ctx.h, vp(d_plane), args[1], width, *args[2:]) == -1, k
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, *good[:5], vp(host_c.ctypes.data + 1), p(host_e)) == -1
        assert se(ctx.h, vp(d_plane + 4), 2, width, *good[2:]) == -1 and se(ctx.h, None, 2, width, *good[2:]) == -1
        assert se(None, vp(d_plane), 2, width, *good[2:]) == -1
        assert se(ctx.h, vp(d_plane), 2, -1, *good[2:]) == -1
        assert pw(ctx.h, vp(d_plane + 4), n, width, *good) == -1 and pw(ctx.h, None, n, width, *good) == -1
        assert pw(ctx.h, vp(d_plane), 0, width, *good) == -1 and pw(ctx.h, vp(d_plane), n, -1, *good) == -1
        assert ex(plan.h, None, data.size, width, *good) == -1 and ex(plan.h, vp(d_in), data.size, -1, *good) == -1
        assert L.sp_plan_bursts_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
        counts, edges = out.read("refusals")
        assert (counts.view(np.uint8) == GARBAGE).all() and (edges.view(np.uint8) == GARBAGE).all()     # nothing was written by any
        assert (host_c == 7).all() and (host_e == 7).all()
        # ... and what is allowed: lo == hi, 4 bytes of alignment, a negative lo
        assert ex(plan.h, vp(d_in), data.size, width, ok_b, 2, ok_h, dbl(-1.0, 4.0), 3, vp(out.counts + 4), vp(out.edges + 4)) == 0
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok_b, 2, ok_h, ok_l, 4, p(host_c), p(host_e)) == 0
        ctx.synchronize()
        assert (host_c[2:] == 7).all() and (host_e[16:] == 7).all() and (host_c[:2] <= width).all()
    finally:
        peak.close()
        plan.close()
        out.free()
        for p_ in (d_in, d_plane):
            ctx.free(p_)


# ---- (f) interleaving, also under stream capture -------------------------------------------------------------------------------------------------
def _interleave_reference(fmt, n, width):
    data, win, bn, bands, hi, lo, want = _oracle_reference(fmt, n, width, False)
    plane = _hop_reference(fmt, n, width, False, n // 2 + 3)[3]
    return data, win, bn, bands, hi, lo, want, plane


@pytest.mark.parametrize("fmt,n,width", [("CS16", 256, 300), ("CU8", 2048, 37)])
def test_bursts_interleave_without_a_synchronisation(ctx, fmt, n, width):
    """sp_plan_execute_bursts, sp_plan_execute, _power, _mean, _bandpower, _quantile and _bursts again on one context without a
    synchronisation; between them a request of another capture whose workspace is smaller (37 frames against 300) or larger."""
    data, win, bn, bands, hi, lo, want, plane = _interleave_reference(fmt, n, width)
    other_w = 300 if width < 300 else 37
    o_data, _, _, _, o_hi, o_lo, o_want, _ = _interleave_reference(fmt, n, other_w)
    ranks = [quantileref.rank_of(width, 0.5)]
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    r_want = pyoracle.render(fmt, data, n, win, bn, 3.0, 50.0, lut, width)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, lut)
    d_in, d_other = _upload(ctx, data), _upload(ctx, o_data)
    sizes = [4 * width * n, width, width, width, 8 * 256, 8000, 16]
    first = [ctx.alloc(s_) for s_ in sizes]
    b1, b2, b_other = (_Words(ctx, len(bands), 12) for _ in range(3))
    m_out, p_out, s_out, q_out = _Out(ctx, n), _Out(ctx, width * n), _Out(ctx, len(bands) * width), _Out(ctx, n)
    from test_gpu_parity import _assert_same as assert_same_reply
    try:
        for p_, s_ in zip(first, sizes):
            ctx.memset(p_, 0xA5, s_)
        ctx.synchronize()
        plan.execute_bursts(d_in, data.size, width, bands, hi, lo, 12, b1.counts, b1.edges)
        plan.execute(d_in, data.size, width, *first)
        plan.execute_power(d_in, data.size, width, p_out.ptr)
        plan.execute_mean(d_in, data.size, width, m_out.ptr)
        plan.execute_bursts(d_other, o_data.size, other_w, bands, o_hi, o_lo, 12, b_other.counts, b_other.edges)
        plan.execute_bandpower(d_in, data.size, width, bands, s_out.ptr)
        plan.execute_quantile(d_in, data.size, width, ranks, q_out.ptr)
        plan.execute_bursts(d_in, data.size, width, bands, hi, lo, 12, b2.counts, b2.edges)
        ctx.synchronize()
        got = {"rgba": ctx.download(first[0], sizes[0]), "gauge_mins": ctx.download(first[1], width),
               "gauge_maxs": ctx.download(first[2], width), "gauge_amps": ctx.download(first[3], width),
               "c_hist": ctx.download(first[4], 8 * 256, np.uint64), "cB_hist": ctx.download(first[5], 8000, np.uint64)}
        mm = ctx.download(first[6], 16, np.float64)
        got["dBfs_min"], got["dBfs_max"] = float(mm[0]), float(mm[1])
        assert_same_reply(got, r_want)
        powerref.assert_same(p_out.read("power").reshape(width, n), plane, "the plane between them")
        meanref.assert_same(m_out.read("mean"), meanref.expected(plane), "the mean between them")
        bandref.assert_same(s_out.read("bands").reshape(len(bands), width), bandref.expected(plane, bands), "the band sums between them")
        quantileref.assert_same(q_out.read("median").view(np.uint64).reshape(1, n), quantileref.expected(plane, ranks), "the median")
        assert_same(b1.read("first"), want, "first")
        assert_same(b_other.read("other"), o_want, "a smaller or larger workspace")
        assert_same(b2.read("again"), want, "again")
    finally:
        for o in (b1, b2, b_other, m_out, p_out, s_out, q_out):
            o.free()
        for p_ in first + [d_in, d_other]:
            ctx.free(p_)
        plan.close()


def test_bursts_are_captured_between_their_neighbours_and_replayed(pkg):
    """The entry points without a request number - _power, _mean, _bandpower, _quantile and _bursts, a smaller request of _bursts
    between two larger ones - captured into one hipGraph on a stream of the context's, after a run outside the capture that leaves the
    workspaces at their sizes; the graph is launched once and every reply is the reference's."""
    hip = _hip_runtime(pkg)
    fmt, n, width = "CS16", 256, 300
    data, win, bn, bands, hi, lo, want, plane = _interleave_reference(fmt, n, width)
    o_data, _, _, _, o_hi, o_lo, o_want, _ = _interleave_reference(fmt, n, 37)
    ranks = [quantileref.rank_of(width, 0.5)]
    own = pkg.Context(0)
    stream, graph, exe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        plan = own.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
        d_in, d_other = _upload(own, data), _upload(own, o_data)
        b1, b2, b_other = (_Words(own, len(bands), 12) for _ in range(3))
        m_out, p_out, s_out, q_out = _Out(own, n), _Out(own, width * n), _Out(own, len(bands) * width), _Out(own, n)
        assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
        own.set_stream(stream.value)

        def queue():
            plan.execute_bursts(d_in, data.size, width, bands, hi, lo, 12, b1.counts, b1.edges)
            plan.execute_power(d_in, data.size, width, p_out.ptr)
            plan.execute_mean(d_in, data.size, width, m_out.ptr)
            plan.execute_bursts(d_other, o_data.size, 37, bands, o_hi, o_lo, 12, b_other.counts, b_other.edges)
            plan.execute_bandpower(d_in, data.size, width, bands, s_out.ptr)
            plan.execute_quantile(d_in, data.size, width, ranks, q_out.ptr)
            plan.execute_bursts(d_in, data.size, width, bands, hi, lo, 12, b2.counts, b2.edges)

        queue()                                                        # (outside a capture: the workspaces exist from here on)
        own.synchronize()
        for o in (b1, b2, b_other):
            for base, size in zip(o.base, o.sizes):
                own.memset(base, GARBAGE, size + 2 * GUARD)
        own.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0               # hipStreamCaptureModeThreadLocal
        try:
            queue()
        finally:
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
        assert graph.value
        assert (b1.read("recorded, not run")[0].view(np.uint8) == GARBAGE).all()
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
        assert hip.hipGraphLaunch(exe, stream) == 0
        own.synchronize()
        assert_same(b1.read("first"), want, "captured: first")
        assert_same(b_other.read("other"), o_want, "captured: the smaller request")
        assert_same(b2.read("again"), want, "captured: again")
        bandref.assert_same(s_out.read("bands").reshape(len(bands), width), bandref.expected(plane, bands), "captured: the band sums")
        meanref.assert_same(m_out.read("mean"), meanref.expected(plane), "captured: the mean")
        plan.close()
        for o in (b1, b2, b_other, m_out, p_out, s_out, q_out):
            o.free()
        for p_ in (d_in, d_other):
            own.free(p_)
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        own.set_stream(None)
        own.close()
        if stream.value:
            hip.hipStreamDestroy(stream)
