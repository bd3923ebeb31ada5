"""The burst measurements on the GPU (sp_series_pulses, sp_power_pulses, sp_plan_execute_pulses, sp_render_pulses): every comparison is
of whole arrays, bit for bit, against tests/pulseref.py - burstref's bursts, math.fsum and a plain loop per burst - on pulseref's planted
series, on bandref's exact band sums of a synthetic plane, or on those of the oracle's plane.  Every result lies between guard bytes and
holds garbage before the call.  There is no tolerance anywhere.

The measurement that goes with the feature is not asserted here (tools/pulse_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bandref
import powerref
import pulseref
from oracle import pyoracle
from test_bursts_gpu import S, WIDTHS_A, _band_sums, _execute_bursts, _gated_plane, _interleave_reference, _oracle_reference
from test_density_gpu import _hip_runtime
from test_mean_gpu import FORMATS, GARBAGE, GUARD, KERNELS, _capture, _Out, _reference, _upload
from test_track_gpu import _hop_reference
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

NAMES = ("counts", "edges", "energy", "peak", "peak_at")
ALL = frozenset(NAMES)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Five:
    """The five device outputs - counts uint32 [count], edges int32 [count, m, 2], energy and peak f64 [count, m] (read as uint64 bits)
    and peak_at int32 [count, m] - each between two guards, everything garbage; an output not in `which` is passed as NULL."""

    def __init__(self, ctx, count, m, which=ALL):
        self.ctx, self.count, self.m = ctx, count, m
        per = {"counts": 4 * count, "edges": 8 * count * m, "energy": 8 * count * m, "peak": 8 * count * m, "peak_at": 4 * count * m}
        self.sizes = [per[k] if k in which else 0 for k in NAMES]
        self.base = [ctx.alloc(s + 2 * GUARD) for s in self.sizes]
        for b, s in zip(self.base, self.sizes):
            ctx.memset(b, GARBAGE, s + 2 * GUARD)
        self.ptr = [b + GUARD if k in which and (k == "counts" or m > 0) else 0 for b, k in zip(self.base, NAMES)]

    def read(self, what=""):
        out = []
        for b, s, present, k in zip(self.base, self.sizes, self.ptr, NAMES):
            whole = self.ctx.download(b, s + 2 * GUARD)
            assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + s:] == GARBAGE).all(), "%s: bytes around %s were written" % (what, k)
            out.append(whole[GUARD:GUARD + s].copy() if present else None)
        shape = (self.count, self.m)
        view = [(np.uint32, (self.count,)), (np.int32, shape + (2,)), (np.uint64, shape), (np.uint64, shape), (np.int32, shape)]
        return tuple(a.view(t).reshape(sh) if a is not None else None for a, (t, sh) in zip(out, view))

    def garbage(self):
        return all((self.ctx.download(b, s + 2 * GUARD) == GARBAGE).all() for b, s in zip(self.base, self.sizes))

    def free(self):
        for b in self.base:
            self.ctx.free(b)


def as_bits(reply):
    """A host reply (float64 energy and peak) as pulseref's: uint64 bits."""
    counts, edges, energy, peak, peak_at = reply
    return counts, edges, np.ascontiguousarray(energy).view(np.uint64), np.ascontiguousarray(peak).view(np.uint64), peak_at


def assert_same(got, want, what):
    """Whole arrays for equality; a None on the left is an output that was not asked for."""
    for g, w, name in zip(got, want, NAMES):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %r %r, want %r %r" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            at = tuple(np.argwhere(g != w)[0])
            raise AssertionError("%s: the %s differ in %d of %d words, first at %r: got %r, want %r"
                                 % (what, name, int((g != w).sum()), w.size, at, g[at], w[at]))


def _series_pulses(ctx, d_series, count, width, hi, lo, m, what, which=ALL):
    out = _Five(ctx, count, m, which)
    try:
        ctx.series_pulses(d_series if count * width else 0, count, width, hi, lo, m, *out.ptr)
        ctx.synchronize()
        got = out.read(what)
        assert all((g is None) == (k not in which or (k != "counts" and m == 0)) for g, k in zip(got, NAMES))
        return got
    finally:
        out.free()


def _cutting(full, width):
    """max_bursts that cuts inside a segment: burst max_bursts - 1 of some band spans a segment boundary and burst max_bursts exists;
    None where the expected bursts of the shape hold no such burst."""
    counts, edges = full[0], full[1]
    for b in range(len(counts)):
        for i in range(int(counts[b]) - 1):
            s, e = edges[b, i]
            if s // S != (e - 1) // S:
                return i + 1
    return None


# ---- (a) sp_series_pulses on planted series ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS_A, ids=["W%d" % w for w in WIDTHS_A])
def test_series_pulses_of_planted_series(ctx, width):
    """Six bands, one per role of burstref.ROLES; max_bursts with room for every burst, and one that cuts inside a segment (7 where the
    shape has no burst across a segment boundary that another one follows); every output alone and all together.  What the series
    holds is asserted on the reference's output (pulseref.telling) before anything runs."""
    for seed in (0, 1) if width <= 257 else (0,):
        count = 6
        series, hi, lo = pulseref.planted_series(seed, count, width, S)
        assert pulseref.must_tell(seed, count, width, S) <= pulseref.telling(seed, count, width, S), (seed, width)
        full = pulseref.planted_expected(seed, count, width, S)
        cutting = _cutting(full, width)
        assert cutting is not None or width < 2 * S + 3, width
        d_series = _upload(ctx, series)
        try:
            for m in (width // 2 + 1, cutting or 7):
                want = pulseref.cut(full, m)
                what = "sp_series_pulses seed %d W=%d max_bursts %d" % (seed, width, m)
                if m == cutting:
                    assert (want[0] > m).any() and (want[4][want[0] > m, m - 1] >= 0).all(), what       # cut, and the last slot is measured
                assert_same(_series_pulses(ctx, d_series, count, width, hi, lo, m, what), want, what)
                for k in NAMES:
                    assert_same(_series_pulses(ctx, d_series, count, width, hi, lo, m, what, frozenset([k])), want, what + ": %s alone" % k)
        finally:
            ctx.free(d_series)


def test_series_pulses_reads_values_by_key_and_max_bursts_0_counts(ctx):
    """The sign bit of a value is not looked at: the negated series gives the same words.  With max_bursts == 0 the per-burst outputs
    count as absent: the counts are written and nothing else."""
    series, hi, lo = pulseref.planted_series(0, 6, 300, S)
    full = pulseref.planted_expected(0, 6, 300, S)
    d = _upload(ctx, -series)
    try:
        assert_same(_series_pulses(ctx, d, 6, 300, hi, lo, 9, "negated"), pulseref.cut(full, 9), "negated")
        out = _Five(ctx, 6, 3)
        ctx.series_pulses(d, 6, 300, hi, lo, 0, *out.ptr)
        ctx.synchronize()
        got = out.read("max_bursts 0")
        assert np.array_equal(got[0], full[0]) and all((g.view(np.uint8) == GARBAGE).all() for g in got[1:])
        out.free()
    finally:
        ctx.free(d)


# ---- (b) sp_power_pulses on a synthetic plane --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", [(2, 300), (100, S + 1), (256, 300)])
def test_power_pulses_of_a_synthetic_plane(ctx, n, width):
    """sp_power_pulses == sp_series_pulses of sp_power_bands of the same plane == pulseref of bandref's exact sums."""
    plane, bands, sums, hi, lo = _gated_plane(n, width)
    m = 16
    want = pulseref.expected(sums, hi, lo, m)
    assert (want[0] > 2).sum() >= 3 and want[0][0] == 1 and (want[1][0, 0] == (0, width)).all()
    count = len(bands)
    d_p, d_s = _upload(ctx, plane), ctx.alloc(8 * count * width)
    direct, chained = _Five(ctx, count, m), _Five(ctx, count, m)
    try:
        ctx.power_pulses(d_p, n, width, bands, hi, lo, m, *direct.ptr)
        ctx.power_bands(d_p, n, width, bands, d_s)
        ctx.series_pulses(d_s, count, width, hi, lo, m, *chained.ptr)
        ctx.synchronize()
        assert_same(direct.read("direct"), want, "sp_power_pulses n=%d W=%d" % (n, width))
        assert_same(chained.read("chained"), want, "sp_series_pulses of sp_power_bands")
    finally:
        for o in (direct, chained):
            o.free()
        for p_ in (d_p, d_s):
            ctx.free(p_)


# ---- (c) sp_plan_execute_pulses against the oracle's plane ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_pulses(fmt, n, width, ch, m=12):
    """test_bursts_gpu's oracle request - the thresholds are every band series' own median times 4 and times 2 - and pulseref on
    bandref's sums of the oracle's plane."""
    data, win, bn, bands, hi, lo, burst_want = _oracle_reference(fmt, n, width, ch)
    plane = _hop_reference(fmt, n, width, ch, n // 2 + 3)[3]
    want = pulseref.expected(bandref.expected(plane, bands), hi, lo, m)
    assert np.array_equal(want[0], burst_want[0]) and np.array_equal(want[1], burst_want[1])
    for a in want:
        a.setflags(write=False)
    return data, win, bn, bands, hi, lo, want


def _execute_pulses(ctx, plan, d_in, nbytes, width, bands, hi, lo, m, what):
    out = _Five(ctx, len(bands), m)
    try:
        plan.execute_pulses(d_in, nbytes, width, bands, hi, lo, m, *out.ptr)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


ORACLE_WIDTHS = (2, 37)


@pytest.mark.parametrize("k", range(len(KERNELS)), ids=["n%d%s" % (n, "-forced" if f else "") for n, f, _ in KERNELS])
@pytest.mark.parametrize("width", ORACLE_WIDTHS, ids=["W%d" % w for w in ORACLE_WIDTHS])
def test_execute_pulses_against_the_oracle(ctx, k, width):
    """Every (kernel, n) of the mean's oracle test; the format and the channel mode rotate as there.  counts and edges are also the
    reply of sp_plan_execute_bursts on the same request."""
    n, forced, name = KERNELS[k]
    j = ORACLE_WIDTHS.index(width)
    fmt, ch = FORMATS[(k + j) % 3], (k // 3 + j) % 2 == 1
    data, win, bn, bands, hi, lo, want = _oracle_pulses(fmt, n, width, ch)
    what = "%s n=%d W=%d%s%s" % (fmt, n, width, " L/R" if ch else "", " forced" if forced else "")
    if width >= 37:
        assert (want[0] > 0).any() and (want[4] >= 0).any(), what
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.pulses_kernel_name_for(data.size, width) == name + "+pulses"
        got = _execute_pulses(ctx, plan, d_in, data.size, width, bands, hi, lo, 12, what)
        assert_same(got, want, what)
        bursts = _execute_bursts(ctx, plan, d_in, data.size, width, bands, hi, lo, 12, what)
        assert np.array_equal(got[0], bursts[0]) and np.array_equal(got[1], bursts[1]), what
    finally:
        ctx.free(d_in)
        plan.close()


# ---- (d) independence of the window, the chunking and the layout -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 256, 300, False), ("CF32", 1024, 37, True)])
def test_the_window_and_the_layout_do_not_change_a_word(ctx, fmt, n, width, ch):
    data, win, bn, bands, hi, lo, want = _oracle_pulses(fmt, n, width, ch)
    assert (want[0] > 0).any()
    d_in = _upload(ctx, data)
    got = []
    try:
        for waterfall in (False, True):
            plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch, waterfall)
            try:
                for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, one byte (one frame), the default
                    ctx.set_mean_window(window)
                    got.append(_execute_pulses(ctx, plan, d_in, data.size, width, bands, hi, lo, 12, "window %d" % window))
            finally:
                ctx.set_mean_window(0)
                plan.close()
    finally:
        ctx.free(d_in)
    for g in got:
        assert_same(g, want, "window / layout")


def test_chunked_sp_render_pulses_whose_chunks_cut_a_burst(ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts, on multiples of 32 frames: a burst that runs over all frames (the
    band of every row against hi = 0) and the median's bursts of the other bands, with the default window and with one of five frames."""
    fmt, n, width = "CF32", 1024, 2048
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n)
    bands = [(0, n), (0, 1), (n // 4, n // 2), (5, 5)]
    sums = _band_sums(fmt, n, width, tuple(bands))
    median = np.sort(sums, axis=1)[:, (width - 1) // 2]
    hi, lo = 1.25 * median, 0.8 * median
    hi[0] = lo[0] = 0.0
    want = pulseref.expected(sums, hi, lo, 40)
    assert want[0][0] == 1 and (want[1][0, 0] == (0, width)).all()
    assert any(s >= 0 and s // 32 != (e - 1) // 32 for s, e in want[1][1:].reshape(-1, 2)), "no burst crosses a multiple of 32 frames"
    try:
        ctx.set_mean_window(5 * 8 * n)
        got = ctx.render_pulses(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, 40, fill=GARBAGE)
        assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    finally:
        ctx.set_mean_window(0)
    assert_same(as_bits(got), want, "a window of five frames")
    default = ctx.render_pulses(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, 40, fill=GARBAGE)
    assert ctx.last_chunks() > 1
    assert_same(as_bits(default), want, "the default window")


def test_small_sparse_request_into_host_arrays_between_guards(pkg, ctx):
    """sp_render_pulses into host arrays between guards, every output and each alone; a number for hi and lo is every band's."""
    fmt, n, width = "CU8", 256, 64
    data, win, bn, plane, _ = _hop_reference(fmt, n, width, False, 40 * n + 11)
    bands = bandref.standard_bands(n)
    sums = bandref.expected(plane, bands)
    hi = float(np.median(sums[1]) * 4.0)
    lo = hi / 4
    m, count = 5, len(bands)
    want = pulseref.expected(sums, [hi] * count, [lo] * count, m)
    assert want[0][1] >= 2 and want[0][0] == 0
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, False, False)
    b = np.ascontiguousarray(bands, np.int32)
    h, l = np.full(count, hi), np.full(count, lo)
    sizes = (4 * count, 8 * count * m, 8 * count * m, 8 * count * m, 4 * count * m)
    types = ((np.uint32, (count,)), (np.int32, (count, m, 2)), (np.uint64, (count, m)), (np.uint64, (count, m)), (np.int32, (count, m)))
    vp = C.c_void_p
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    for which in [ALL] + [frozenset([k]) for k in NAMES]:
        host = [np.full(s + 2 * GUARD, GARBAGE, np.uint8) for s in sizes]
        args = [vp(a.ctypes.data + GUARD) if k in which else None for a, k in zip(host, NAMES)]
        assert ctx.lib.L.sp_render_pulses(ctx.h, C.byref(req), p(data), data.size, width, p(b), count, p(h), p(l), m, *args) == 0
        got = []
        for a, s, k, (t, sh) in zip(host, sizes, NAMES, types):
            assert (a[:GUARD] == GARBAGE).all() and (a[GUARD + s:] == GARBAGE).all()
            if k in which:
                got.append(a[GUARD:GUARD + s].view(t).reshape(sh))
            else:
                assert (a == GARBAGE).all()
                got.append(None)
        assert_same(got, want, "sparse sp_render_pulses %s" % sorted(which))
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1
    assert_same(as_bits(ctx.render_pulses(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, m, fill=GARBAGE)), want, "scalar thresholds")


# ---- (e) no frames, no bands, refusals ---------------------------------------------------------------------------------------------------------
def _filled(got):
    return (got[0] == 0).all() and all((g.view(np.uint8) == 0xFF).all() for g in got[1:] if g is not None)


def test_width_0_and_count_0(pkg, ctx):
    n = 128
    data = _capture("CU8", n, 20, 3 * n)
    win, weight = pyoracle.window("hann", n)
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, data)
    bands = [(0, n), (3, 9), (0, 0)]
    try:
        for m in (0, 4):
            out = _Five(ctx, 3, m)
            plan.execute_pulses(d_in, data.size, 0, bands, 2.0, 1.0, m, *out.ptr)          # width == 0
            ctx.synchronize()
            assert _filled(out.read("width 0"))
            out.free()
        out = _Five(ctx, 3, 4)
        ctx.power_pulses(0, n, 0, bands, 2.0, 1.0, 4, *out.ptr)
        ctx.synchronize()
        assert _filled(out.read("width 0, a plane"))
        out.free()
        out = _Five(ctx, 3, 4)
        ctx.series_pulses(0, 3, 0, 2.0, 1.0, 4, *out.ptr)
        ctx.synchronize()
        assert _filled(out.read("width 0, a series"))
        out.free()
        out = _Five(ctx, 3, 4)                                                             # count == 0: nothing is written
        plan.execute_pulses(d_in, data.size, 20, [], 2.0, 1.0, 4, *out.ptr)
        ctx.series_pulses(d_in, 0, 20, 2.0, 1.0, 4, *out.ptr)
        ctx.synchronize()
        assert out.garbage()
        out.free()
    finally:
        ctx.free(d_in)
        plan.close()
    got = ctx.render_pulses("CU8", data, n, win, 1.0 / weight, 3.0, 50.0, 0, bands, 2.0, 1.0, 4, fill=GARBAGE)
    assert got[2].shape == (3, 4) and got[4].shape == (3, 4) and _filled(as_bits(got))
    got = ctx.render_pulses("CU8", data, n, win, 1.0 / weight, 3.0, 50.0, 20, [], 2.0, 1.0, 4, fill=GARBAGE)
    assert all(g.size == 0 for g in got)


def test_refusals(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    d_in, d_plane = ctx.alloc(data.size), ctx.alloc(8 * width * n + 16)
    out = _Five(ctx, 4, 4)
    vp = C.c_void_p
    nan = float("nan")

    def ints(*v):
        return (C.c_int32 * len(v))(*v)

    def dbl(*v):
        return (C.c_double * len(v))(*v)

    ok_b, ok_h, ok_l = ints(0, n, 3, 9), dbl(4.0, 4.0), dbl(1.0, 4.0)
    ptrs = tuple(vp(p_) for p_ in out.ptr)
    # (bands, count, hi, lo, max_bursts, counts, edges, energy, peak, peak_at)
    good = (ok_b, 2, ok_h, ok_l, 4) + ptrs

    def moved(k, by):
        return good[:5 + k] + (vp(out.ptr[k] + by),) + good[6 + k:]

    bad = [(ints(0, n + 1, 3, 9),) + good[1:], (ints(5, 4, 3, 9),) + good[1:], (ints(-1, 4, 3, 9),) + good[1:],          # bad bands
           (None,) + good[1:], (ok_b, -1) + good[2:], (ints(*([0, 1] * 65)), 65, dbl(*([4.0] * 65)), dbl(*([1.0] * 65))) + good[4:],
           good[:2] + (dbl(4.0, nan),) + good[3:], good[:3] + (dbl(nan, 1.0),) + good[4:],                              # a NaN threshold
           good[:3] + (dbl(1.0, 4.5),) + good[4:], good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:],         # lo > hi; none
           good[:4] + (-1,) + good[5:], good[:4] + (2 ** 29,) + good[5:],                                               # max_bursts
           good[:5] + (None,) * 5, good[:4] + (0, None) + good[6:],                                                    # every output absent
           moved(0, 2), moved(1, 1), moved(2, 4), moved(3, 4), moved(4, 2)]                                             # misaligned
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "peak")
    host = (np.full(4, 7, np.uint32), np.full(32, 7, np.int32), np.full(16, 7.0), np.full(16, 7.0), np.full(16, 7, np.int32))
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_pulses(d_in, data.size, width, [(0, n)], 4.0, 1.0, 4, *out.ptr)
        assert e.value.status == -4 and "peak" in str(e.value)
        ex, pw, se, rt = L.sp_plan_execute_pulses, L.sp_power_pulses, L.sp_series_pulses, L.sp_render_pulses
        host_ptrs = tuple(p(a) for a in host)
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok_b, 2, ok_h, ok_l, 4, *host_ptrs) == -4
        req.detector = 0
        assert ex(None, vp(d_in), data.size, width, *good) == -1
        for k, args in enumerate(bad):
            assert ex(plan.h, vp(d_in), data.size, width, *args) == -1, k
            assert pw(ctx.h, vp(d_plane), n, width, *args) == -1, k
            if k < len(bad) - 5:
                on_host = args[:5] + tuple(a if a is None else h for a, h in zip(args[5:], host_ptrs))
                assert rt(ctx.h, C.byref(req), p(data), data.size, width, *on_host) == -1, k
            if k >= 4:                                                       # (the series has no bands)
                assert se(ctx.h, vp(d_plane), args[1], width, *args[2:]) == -1, k
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, *good[:5], *host_ptrs[:2], vp(host[2].ctypes.data + 4), *host_ptrs[3:]) == -1
        assert se(ctx.h, vp(d_plane + 4), 2, width, *good[2:]) == -1 and se(ctx.h, None, 2, width, *good[2:]) == -1
        assert se(None, vp(d_plane), 2, width, *good[2:]) == -1 and se(ctx.h, vp(d_plane), 2, -1, *good[2:]) == -1
        assert pw(ctx.h, vp(d_plane + 4), n, width, *good) == -1 and pw(ctx.h, None, n, width, *good) == -1
        assert pw(ctx.h, vp(d_plane), 0, width, *good) == -1 and pw(ctx.h, vp(d_plane), n, -1, *good) == -1
        assert ex(plan.h, None, data.size, width, *good) == -1 and ex(plan.h, vp(d_in), data.size, -1, *good) == -1
        assert L.sp_plan_pulses_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
        assert out.garbage()                                                 # nothing was written by any
        assert all((a == 7).all() for a in host)
        # ... and what is allowed: lo == hi, 4 bytes of alignment for the int arrays, a negative lo, energy alone
        assert ex(plan.h, vp(d_in), data.size, width, ok_b, 2, ok_h, dbl(-1.0, 4.0), 3, vp(out.ptr[0] + 4), vp(out.ptr[1] + 4), ptrs[2], ptrs[3],
                  vp(out.ptr[4] + 4)) == 0
        assert ex(plan.h, vp(d_in), data.size, width, ok_b, 2, ok_h, ok_l, 3, None, None, ptrs[2], None, None) == 0
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok_b, 2, ok_h, ok_l, 4, *host_ptrs) == 0
        ctx.synchronize()
        assert (host[0][2:] == 7).all() and (host[1][16:] == 7).all() and (host[2][8:] == 7).all() and (host[0][:2] <= width).all()
    finally:
        peak.close()
        plan.close()
        out.free()
        for p_ in (d_in, d_plane):
            ctx.free(p_)


# ---- (f) interleaving, also under stream capture -------------------------------------------------------------------------------------------------
def _interleave_pulses(fmt, n, width):
    data, win, bn, bands, hi, lo, burst_want, plane = _interleave_reference(fmt, n, width)
    want = _oracle_pulses(fmt, n, width, False)[6]
    return data, win, bn, bands, hi, lo, burst_want, want, plane


@pytest.mark.parametrize("fmt,n,width", [("CS16", 256, 300), ("CU8", 2048, 37)])
def test_pulses_interleave_without_a_synchronisation(ctx, fmt, n, width):
    """sp_plan_execute_pulses, _power, _bandpower, _bursts and _pulses again on one context without a synchronisation; between them a
    request of another capture whose workspaces are smaller (37 frames against 300, 5 slots against 12) or larger."""
    data, win, bn, bands, hi, lo, burst_want, want, plane = _interleave_pulses(fmt, n, width)
    other_w = 300 if width < 300 else 37
    o_data, _, _, _, o_hi, o_lo, _, o_want, _ = _interleave_pulses(fmt, n, other_w)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in, d_other = _upload(ctx, data), _upload(ctx, o_data)
    p1, p2, p_other = _Five(ctx, len(bands), 12), _Five(ctx, len(bands), 12), _Five(ctx, len(bands), 5)
    b_out = _Five(ctx, len(bands), 12, frozenset(["counts", "edges"]))
    p_out, s_out = _Out(ctx, width * n), _Out(ctx, len(bands) * width)
    try:
        plan.execute_pulses(d_in, data.size, width, bands, hi, lo, 12, *p1.ptr)
        plan.execute_power(d_in, data.size, width, p_out.ptr)
        plan.execute_pulses(d_other, o_data.size, other_w, bands, o_hi, o_lo, 5, *p_other.ptr)
        plan.execute_bandpower(d_in, data.size, width, bands, s_out.ptr)
        plan.execute_bursts(d_in, data.size, width, bands, hi, lo, 12, b_out.ptr[0], b_out.ptr[1])
        plan.execute_pulses(d_in, data.size, width, bands, hi, lo, 12, *p2.ptr)
        ctx.synchronize()
        powerref.assert_same(p_out.read("power").reshape(width, n), plane, "the plane between them")
        bandref.assert_same(s_out.read("bands").reshape(len(bands), width), bandref.expected(plane, bands), "the band sums between them")
        assert_same(p1.read("first"), want, "first")
        assert_same(p_other.read("other"), pulseref.cut(o_want, 5), "a smaller or larger workspace")
        assert_same(b_out.read("bursts"), burst_want, "the burst lists between them")
        assert_same(p2.read("again"), want, "again")
    finally:
        for o in (p1, p2, p_other, b_out, p_out, s_out):
            o.free()
        for p_ in (d_in, d_other):
            ctx.free(p_)
        plan.close()


def test_pulses_are_captured_between_their_neighbours_and_replayed(pkg):
    """_pulses, _power, a smaller request of _pulses, _bandpower, _bursts and _pulses again captured into one hipGraph on a stream of the
    context's, after a run outside the capture that leaves the workspaces at their sizes; the graph is launched once and every reply is
    the reference's.  Nothing about queues is set."""
    hip = _hip_runtime(pkg)
    fmt, n, width = "CS16", 256, 300
    data, win, bn, bands, hi, lo, burst_want, want, plane = _interleave_pulses(fmt, n, width)
    o_data, _, _, _, o_hi, o_lo, _, o_want, _ = _interleave_pulses(fmt, n, 37)
    own = pkg.Context(0)
    stream, graph, exe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        plan = own.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
        d_in, d_other = _upload(own, data), _upload(own, o_data)
        p1, p2, p_other = _Five(own, len(bands), 12), _Five(own, len(bands), 12), _Five(own, len(bands), 5)
        b_out = _Five(own, len(bands), 12, frozenset(["counts", "edges"]))
        p_out, s_out = _Out(own, width * n), _Out(own, len(bands) * width)
        assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
        own.set_stream(stream.value)

        def queue():
            plan.execute_pulses(d_in, data.size, width, bands, hi, lo, 12, *p1.ptr)
            plan.execute_power(d_in, data.size, width, p_out.ptr)
            plan.execute_pulses(d_other, o_data.size, 37, bands, o_hi, o_lo, 5, *p_other.ptr)
            plan.execute_bandpower(d_in, data.size, width, bands, s_out.ptr)
            plan.execute_bursts(d_in, data.size, width, bands, hi, lo, 12, b_out.ptr[0], b_out.ptr[1])
            plan.execute_pulses(d_in, data.size, width, bands, hi, lo, 12, *p2.ptr)

        queue()                                                        # (outside a capture: the workspaces exist from here on)
        own.synchronize()
        for o in (p1, p2, p_other, b_out):
            for base, size in zip(o.base, o.sizes):
                own.memset(base, GARBAGE, size + 2 * GUARD)
        own.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0               # hipStreamCaptureModeThreadLocal
        try:
            queue()
        finally:
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
        assert graph.value
        assert p1.garbage()                                            # recorded, not run
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
        assert hip.hipGraphLaunch(exe, stream) == 0
        own.synchronize()
        assert_same(p1.read("first"), want, "captured: first")
        assert_same(p_other.read("other"), pulseref.cut(o_want, 5), "captured: the smaller request")
        assert_same(b_out.read("bursts"), burst_want, "captured: the burst lists")
        assert_same(p2.read("again"), want, "captured: again")
        bandref.assert_same(s_out.read("bands").reshape(len(bands), width), bandref.expected(plane, bands), "captured: the band sums")
        plan.close()
        for o in (p1, p2, p_other, b_out, p_out, s_out):
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
