"""The peak track on the GPU (sp_power_tracks, sp_plan_execute_track, sp_render_track): every comparison is exact against
tests/trackref.py - numpy's argmax over the values of a band that are not NaN, the first of equal maxima - on the oracle's plane
(tests/powerref.py) or on a synthetic one that plants ties, neighbouring bit patterns, NaNs and infinities: the rows equal, the peaks
bit for bit (which NaN a NaN is, is the one thing left uncompared).  Every result lies between guard bytes and holds garbage before the
call.

A fixed tone never moves its peak, so the captures here hop: eight segments of the tests' trinoise generator with eight tone steps.

The measurement that goes with the feature is not asserted here (tools/track_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bandref
import meanref
import powerref
import siggen
import trackref
from __graft_entry__ import load_package
from oracle import pyoracle
from test_gpu_parity import _assert_same as assert_same_reply
from test_mean_gpu import FORMATS, GARBAGE, GEN, GUARD, KERNELS, WIDTHS, _capture, _reference, _upload

pytestmark = pytest.mark.gpu

STEPS = (5003, 60001, 12289, 40961, 22003, 51001, 3001, 33331)
NOISE = {"kind": "bytes", "seed": 9001}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Out:
    """Two device arrays, int32 [count, width] and f64 [count, width], each between two guards, everything garbage."""

    def __init__(self, ctx, count, width):
        self.ctx, self.shape = ctx, (count, width)
        self.sizes = (4 * count * width, 8 * count * width)
        self.bases = [ctx.alloc(s + 2 * GUARD) for s in self.sizes]
        assert all(b % 8 == 0 for b in self.bases)
        self.row, self.peak = (b + GUARD for b in self.bases)
        for b, s in zip(self.bases, self.sizes):
            ctx.memset(b, GARBAGE, s + 2 * GUARD)

    def whole(self):
        return [self.ctx.download(b, s + 2 * GUARD) for b, s in zip(self.bases, self.sizes)]

    def read(self, what=""):
        """(rows, peaks); the guards of both arrays must be intact."""
        out = []
        for whole, s, dt in zip(self.whole(), self.sizes, (np.int32, np.float64)):
            assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + s:] == GARBAGE).all(), what + ": bytes around the track were written"
            out.append(whole[GUARD:GUARD + s].view(dt).reshape(self.shape).copy())
        return tuple(out)

    def free(self):
        for b in self.bases:
            self.ctx.free(b)


def _power_tracks(ctx, plane, bands, what, rows=True, peaks=True):
    """sp_power_tracks of a host plane f64 [width, n] through a device copy; an output that is not asked for stays garbage."""
    width, n = plane.shape
    d_p, out = _upload(ctx, plane), _Out(ctx, len(bands), width)
    try:
        ctx.power_tracks(d_p if width else 0, n, width, bands, out.row if rows else 0, out.peak if peaks else 0)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_p)
        out.free()


def _execute_track(ctx, plan, d_in, nbytes, width, bands, what):
    out = _Out(ctx, len(bands), width)
    try:
        plan.execute_track(d_in, nbytes, width, bands, out.row, out.peak)
        ctx.synchronize()
        return out.read(what)
    finally:
        out.free()


def hopping(fmt, samples):
    """`samples` samples of a tone that hops: eight trinoise segments of equal length, one tone step each."""
    c = -(-samples // len(STEPS))
    parts = [siggen.generate(fmt, dict(GEN, step=s), c, t0=k * c) for k, s in enumerate(STEPS)]
    return np.concatenate(parts)[:samples * siggen.SAMPLE_WIDTH[fmt.upper()]].copy()


@functools.lru_cache(maxsize=None)
def _hop_reference(fmt, n, width, ch, stride, noise=False):
    """(capture, taper, block_norm, the oracle's plane, (rows, peaks) of bandref.standard_bands(n)) of a hopping capture - or of a
    capture of random bytes - computed once and shared."""
    samples = n + (max(width, 1) - 1) * stride
    data = siggen.generate(fmt, NOISE, samples) if noise else hopping(fmt, samples)
    win, weight = pyoracle.window("hann", n)
    plane = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, ch)["power"]
    what = "%s n=%d W=%d" % (fmt, n, width)
    powerref.assert_telling(plane[:, 1:] if ch else plane, what)
    want = trackref.expected(plane, bandref.standard_bands(n))
    # the reference alone moves its peak and holds no tie, so the rows are a telling reference and do not hang on the tie rule
    full = plane[:, 1:] if ch else plane
    assert all(int((full[x] == full[x].max()).sum()) == 1 for x in range(width)), what + ": a frame of the reference holds a tie"
    if width >= 37:
        assert len(np.unique(want[0][2])) >= 8, what + ": the reference's peak does not move"
    for a in (data, win, plane) + want:
        a.setflags(write=False)
    return data, win, 1.0 / weight, plane, want


# ---- (a) sp_power_tracks on synthetic planes ----------------------------------------------------------------------------------------------
def _bands(n):
    return bandref.standard_bands(n) + [(min(2, n), n)]        # (the last one shifts every row's lane by two)


@functools.lru_cache(maxsize=None)
def _synthetic(n, width):
    plane = trackref.synthetic_plane(9000 * n + width, n, width)
    plane.setflags(write=False)
    want = trackref.expected(plane, _bands(n))
    for a in want:
        a.setflags(write=False)
    return plane, want


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("n", [2, 64, 100, 256])
def test_power_tracks_of_synthetic_planes(ctx, n, width):
    """Planted ties (neighbouring rows, the same lane of two loads, the smaller lane in the later load, all rows equal, all +0.0, row 0
    against row n - 1), pairs that differ in one half of their bits only, DBL_MAX against inf, a denormal against +0.0, NaNs of three
    kinds, an all-NaN band and an inf that must win, on top of frames over the full exponent range; n = 100 is no multiple of a load's
    64 rows, widths 1 and 2 are less than a workgroup's frames, 63, 65 and 257 no multiple of them, 64 is one."""
    plane, want = _synthetic(n, width)
    bands = _bands(n)
    what = "sp_power_tracks n=%d W=%d" % (n, width)
    got = _power_tracks(ctx, plane, bands, what)
    trackref.assert_same(got, want, what)
    rows, peaks = got
    assert (rows[0] == -1).all() and np.isnan(peaks[0]).all()                                  # the empty band
    for b, y in ((1, 0), (5, n - 1)):                                                          # one row: its index, the plane's column
        col = plane[:, y]
        ok = ~np.isnan(col)
        assert (rows[b][ok] == y).all() and (rows[b][~ok] == -1).all()
        assert np.array_equal(peaks[b][ok].view(np.uint64), col[ok].copy().view(np.uint64)) and np.isnan(peaks[b][~ok]).all()
    if width > 16 and n >= 64:
        assert rows[3, 14] == -1 and rows[2, 15] == n // 2 and np.isinf(peaks[2, 16])           # all NaN; the inf wins
    # either output alone: the same array, the other one untouched, the guards intact
    only_rows = _power_tracks(ctx, plane, bands, what + " rows only", peaks=False)
    assert np.array_equal(only_rows[0], rows) and (only_rows[1].view(np.uint8) == GARBAGE).all()
    only_peaks = _power_tracks(ctx, plane, bands, what + " peaks only", rows=False)
    assert (only_peaks[0].view(np.uint8) == GARBAGE).all()
    trackref.assert_same((rows, only_peaks[1]), want, what + " peaks only")


def test_power_tracks_with_the_most_bands(ctx):
    n, width = 100, 65
    plane = _synthetic(n, width)[0]
    bands = [(k, min(n, k + k % 7)) for k in range(bandref.SP_MAX_BANDS)]
    assert len(bands) == 64 and any(y0 == y1 for y0, y1 in bands)
    trackref.assert_same(_power_tracks(ctx, plane, bands, "64 bands"), trackref.expected(plane, bands), "sp_power_tracks with 64 bands")


# ---- (b) sp_plan_execute_track against the oracle's plane -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(KERNELS)), ids=["n%d%s" % (n, "-forced" if f else "") for n, f, _ in KERNELS])
@pytest.mark.parametrize("j", range(len(WIDTHS)), ids=["W%d" % w for w in WIDTHS])
def test_execute_track_against_the_oracle(ctx, k, j):
    """Every (kernel, n) at every width on the hopping capture; the format and the channel mode rotate as in test_mean_gpu.py, so that
    each format and both modes meet each kernel."""
    n, forced, name = KERNELS[k]
    width = WIDTHS[j]
    fmt, ch = FORMATS[(k + j) % 3], (k // 3 + j) % 2 == 1
    data, win, bn, plane, want = _hop_reference(fmt, n, width, ch, n // 2 + 3)
    what = "%s n=%d W=%d%s%s" % (fmt, n, width, " L/R" if ch else "", " forced" if forced else "")
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.track_kernel_name_for(data.size, width) == name + "+track"
        got = _execute_track(ctx, plan, d_in, data.size, width, bandref.standard_bands(n), what)
    finally:
        ctx.free(d_in)
        plan.close()
    trackref.assert_same(got, want, what)
    rows, peaks = got
    assert (rows[5] == n - 1).all() and np.array_equal(peaks[5].view(np.uint64), plane[:, n - 1].copy().view(np.uint64))
    assert (peaks[2] >= peaks[6]).all() and (peaks[2] >= peaks[7]).all() and (peaks[2] > 0).all()    # the whole spectrum holds its parts


def test_execute_track_of_a_noise_capture(ctx):
    """Random bytes as CS16: the peak row differs in most frames."""
    fmt, n, width = "CS16", 256, 300
    data, win, bn, _, want = _hop_reference(fmt, n, width, False, n // 2 + 3, noise=True)
    assert len(np.unique(want[0][2])) > 100
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, data)
    try:
        got = _execute_track(ctx, plan, d_in, data.size, width, bandref.standard_bands(n), "noise")
    finally:
        ctx.free(d_in)
        plan.close()
    trackref.assert_same(got, want, "noise")


# ---- (c) order-freedom ------------------------------------------------------------------------------------------------------------------------
SHAPES = [("CS16", 256, 300, False), ("CF32", 1024, 37, True), ("CU8", 2048, 37, False)]


@pytest.mark.parametrize("fmt,n,width,ch", SHAPES)
def test_the_window_does_not_change_a_bit(ctx, fmt, n, width, ch):
    data, win, bn, _, want = _hop_reference(fmt, n, width, ch, n // 2 + 3)
    bands = bandref.standard_bands(n)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    got = []
    try:
        for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, below one frame (one frame), the default
            ctx.set_mean_window(window)
            got.append(_execute_track(ctx, plan, d_in, data.size, width, bands, "window %d" % window))
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()
    for g in got:
        trackref.assert_same(g, want, "window")
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1].view(np.uint64), got[0][1].view(np.uint64))


# ---- (d) consistency with what exists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", SHAPES)
def test_tracks_of_the_plane_are_the_tracks_of_the_request_and_the_db_form(ctx, fmt, n, width, ch):
    data, win, bn, _, want = _hop_reference(fmt, n, width, ch, n // 2 + 3)
    bands = bandref.standard_bands(n)
    count = len(bands)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in, d_plane = _upload(ctx, data), ctx.alloc(8 * width * n)
    direct, db, from_plane = _Out(ctx, count, width), _Out(ctx, count, width), _Out(ctx, count, width)
    try:
        plan.execute_track(d_in, data.size, width, bands, direct.row, direct.peak)
        plan.power_to_db(direct.peak, count * width, db.peak)
        plan.execute_power(d_in, data.size, width, d_plane)
        ctx.power_tracks(d_plane, n, width, bands, from_plane.row, from_plane.peak)
        ctx.synchronize()
        got, got_db, got_plane = direct.read("direct"), db.read("dB")[1], from_plane.read("from the plane")
    finally:
        for p in (d_in, d_plane):
            ctx.free(p)
        for o in (direct, db, from_plane):
            o.free()
        plan.close()
    trackref.assert_same(got, want, "sp_plan_execute_track")
    assert np.array_equal(got[0], got_plane[0]) and np.array_equal(got[1].view(np.uint64), got_plane[1].view(np.uint64))
    want_db = meanref.db_of(want[1].reshape(-1), bn, 3.0).reshape(want[1].shape)
    bandref.assert_same(got_db, want_db, "sp_plan_power_to_db of the peaks against the oracle's log10")
    assert np.isnan(got_db[0]).all() and np.isfinite(got_db[2]).all()                        # NaN stays NaN
    # ... and the host entry's dB form is the same conversion, beside the same rows
    host_rows, host_db = ctx.render_track(fmt, data, n, win, bn, 3.0, 50.0, width, bands, ch, db=True, fill=GARBAGE)
    assert np.array_equal(host_rows, want[0])
    bandref.assert_same(host_db, got_db, "Context.render_track db")


# ---- (e) the host entry point -------------------------------------------------------------------------------------------------------------------
def _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands, ch=False, db=0):
    """sp_render_track into two host arrays between guards, everything garbage: (status, (rows, peaks), the guards are intact)."""
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, ch, False)
    b = np.ascontiguousarray(np.asarray(bands, np.int32).reshape(-1, 2))
    count, w = b.shape[0], max(width, 0)
    hosts = [np.full(s * count * w + 2 * GUARD, GARBAGE, np.uint8) for s in (4, 8)]
    vp = C.c_void_p
    rc = ctx.lib.L.sp_render_track(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, width, b.ctypes.data_as(vp) if count else None,
                                   count, db, vp(hosts[0].ctypes.data + GUARD), vp(hosts[1].ctypes.data + GUARD))
    intact = all(bool((h[:GUARD] == GARBAGE).all() and (h[h.size - GUARD:] == GARBAGE).all()) for h in hosts)
    rows = hosts[0][GUARD:hosts[0].size - GUARD].view(np.int32).reshape(count, w).copy()
    peaks = hosts[1][GUARD:hosts[1].size - GUARD].view(np.float64).reshape(count, w).copy()
    return rc, (rows, peaks), intact


def test_small_sparse_request_uploads_its_frames_only(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, want = _hop_reference(fmt, n, width, False, 40 * n + 11)
    bands = bandref.standard_bands(n)
    rc, got, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands)
    assert rc == 0 and intact
    trackref.assert_same(got, want, "sparse sp_render_track")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1
    trackref.assert_same(ctx.render_track(fmt, data, n, win, bn, 3.0, 50.0, width, bands, fill=GARBAGE), want, "Context.render_track")
    rc, got_db, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands, db=1)
    assert rc == 0 and intact and np.array_equal(got_db[0], want[0])
    bandref.assert_same(got_db[1], meanref.db_of(want[1].reshape(-1), bn, 3.0).reshape(want[1].shape), "sp_render_track db")


def test_chunked_sp_render_track(pkg, ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts: the capture travels in chunks and every chunk fills its columns.  (The
    plane is the band test's, computed once for both.)"""
    fmt, n, width = "CF32", 1024, 2048
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n)
    bands = bandref.standard_bands(n)
    want = trackref.expected(plane, bands)
    assert data.size >= 16 << 20
    rc, got, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, bands)
    assert rc == 0 and intact
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    trackref.assert_same(got, want, "chunked sp_render_track")


@pytest.mark.parametrize("n", [64, 2048])
def test_capture_shorter_than_n_gives_no_row_and_nan_everywhere(pkg, ctx, n):
    data = siggen.generate("CS16", GEN, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    for db in (0, 1):
        rc, (rows, peaks), intact = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, 3, [(0, n), (1, 2), (n - 1, n), (5, 5)], db=db)
        assert rc == 0 and intact and rows.shape == (4, 3) and (rows == -1).all() and np.isnan(peaks).all()


def test_width_0_and_count_0_write_nothing(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, _ = _hop_reference(fmt, n, width, False, 40 * n + 11)
    vp = C.c_void_p
    # the host entry: its outputs lie inside garbage arrays, of which nothing may change
    for w, bands in ((0, [(0, n), (3, 9)]), (width, [])):
        req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, False, False)
        b = np.asarray(bands, np.int32).reshape(-1, 2)
        host = np.full(4 * GUARD, GARBAGE, np.uint8)
        for row, peak in ((vp(host.ctypes.data + GUARD), vp(host.ctypes.data + 3 * GUARD)), (None, None)):
            assert ctx.lib.L.sp_render_track(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, w,
                                             b.ctypes.data_as(vp) if len(bands) else None, len(bands), 0, row, peak) == 0
        assert (host == GARBAGE).all()
    # the device entries
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in, d_plane, out = _upload(ctx, data), ctx.alloc(8 * width * n), _Out(ctx, 1, 1)
    try:
        plan.execute_track(d_in, data.size, 0, [(0, n)], out.row, out.peak)
        plan.execute_track(d_in, data.size, width, [], out.row, out.peak)
        plan.execute_track(d_in, data.size, 0, [(0, n)], 0, 0)
        plan.execute_track(d_in, data.size, width, [], 0, 0)
        ctx.power_tracks(d_plane, n, 0, [(0, n)], out.row, out.peak)
        ctx.power_tracks(d_plane, n, width, [], out.row, out.peak)
        ctx.power_tracks(0, n, 0, [(0, n)], 0, 0)
        ctx.synchronize()
        assert all((w == GARBAGE).all() for w in out.whole())
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
    d_in, d_row, d_peak, d_plane = ctx.alloc(data.size), ctx.alloc(4 * 64 * width + 16), ctx.alloc(8 * 64 * width + 16), ctx.alloc(8 * width * n + 16)
    vp = C.c_void_p

    def arr(*rows):
        return (C.c_int32 * len(rows))(*rows)

    ok, many = arr(0, n, 3, 9), arr(*([0, 1] * 65))
    bad_bands = [(arr(0, n + 1), 1), (arr(-1, 4), 1), (arr(5, 4), 1), (arr(0, n, n + 1, n + 1), 2), (many, 65), (ok, -1), (None, 1)]
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_track(d_in, data.size, width, [(0, n)], d_row, d_peak)
        assert e.value.status == -4 and "peak" in str(e.value)
        ex = L.sp_plan_execute_track
        assert ex(None, vp(d_in), data.size, width, ok, 2, vp(d_row), vp(d_peak)) == -1
        for bands, count in bad_bands:
            assert ex(plan.h, vp(d_in), data.size, width, bands, count, vp(d_row), vp(d_peak)) == -1, count
            assert L.sp_power_tracks(ctx.h, vp(d_plane), n, width, bands, count, vp(d_row), vp(d_peak)) == -1, count
        assert ex(plan.h, vp(d_in), data.size, width, many, 64, vp(d_row), vp(d_peak)) == 0         # 64 bands are allowed
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, vp(d_row + 2), vp(d_peak)) == -1       # misaligned rows
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, vp(d_row), vp(d_peak + 4)) == -1       # misaligned peaks
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, vp(d_row + 4), vp(d_peak + 8)) == 0    # 4 and 8 bytes are enough
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, None, None) == -1                      # both NULL
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, vp(d_row), None) == 0                  # either one may be
        assert ex(plan.h, vp(d_in), data.size, width, ok, 2, None, vp(d_peak)) == 0
        assert ex(plan.h, vp(d_in), data.size, -1, ok, 2, vp(d_row), vp(d_peak)) == -1
        assert ex(plan.h, None, data.size, width, ok, 2, vp(d_row), vp(d_peak)) == -1
        plan16 = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
        assert ex(plan16.h, vp(d_in), 4 * 100 + 1, width, ok, 2, vp(d_row), vp(d_peak)) == -3
        plan16.close()
        pt = L.sp_power_tracks
        assert pt(None, vp(d_plane), n, width, ok, 2, vp(d_row), vp(d_peak)) == -1
        assert pt(ctx.h, vp(d_plane), 0, width, arr(0, 0), 1, vp(d_row), vp(d_peak)) == -1
        assert pt(ctx.h, vp(d_plane), n, -1, ok, 2, vp(d_row), vp(d_peak)) == -1
        assert pt(ctx.h, vp(d_plane + 4), n, width, ok, 2, vp(d_row), vp(d_peak)) == -1
        assert pt(ctx.h, vp(d_plane), n, width, ok, 2, vp(d_row + 1), vp(d_peak)) == -1
        assert pt(ctx.h, vp(d_plane), n, width, ok, 2, vp(d_row), vp(d_peak + 2)) == -1
        assert pt(ctx.h, vp(d_plane), n, width, ok, 2, None, None) == -1
        assert pt(ctx.h, None, n, width, ok, 2, vp(d_row), vp(d_peak)) == -1
        assert pt(ctx.h, vp(d_plane), 100, width, arr(0, 101), 1, vp(d_row), vp(d_peak)) == -1      # any n >= 1: its own bound
        assert L.sp_plan_track_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
    finally:
        peak.close()
        plan.close()
        for p_ in (d_in, d_row, d_peak, d_plane):
            ctx.free(p_)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "peak")
    rows, peaks = np.zeros(64 * width, np.int32), np.zeros(64 * width)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    rt = L.sp_render_track
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, p(rows), p(peaks)) == -4
    req.detector = 0
    assert rt(None, C.byref(req), p(data), data.size, width, ok, 2, 0, p(rows), p(peaks)) == -1
    assert rt(ctx.h, None, p(data), data.size, width, ok, 2, 0, p(rows), p(peaks)) == -1
    assert rt(ctx.h, C.byref(req), None, data.size, width, ok, 2, 0, p(rows), p(peaks)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, -2, ok, 2, 0, p(rows), p(peaks)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, None, None) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, vp(rows.ctypes.data + 2), p(peaks)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, p(rows), vp(peaks.ctypes.data + 4)) == -1
    for bands, count in bad_bands:
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, bands, count, 0, p(rows), p(peaks)) == -1, count
    assert (rows == 0).all() and (peaks == 0).all()
    req16, keep16 = pkg.binding._make_request(pkg.parse_format("CS16")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False)
    assert rt(ctx.h, C.byref(req16), p(data), 4 * 100 + 1, width, ok, 2, 0, p(rows), p(peaks)) == -3
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, p(rows), None) == 0                 # the rows alone
    assert (peaks == 0).all() and (rows[width:2 * width] >= 3).all() and (rows[width:2 * width] < 9).all() and (rows[2 * width:] == 0).all()
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, ok, 2, 0, p(rows), p(peaks)) == 0
    got = peaks[:2 * width].reshape(2, width)
    assert np.isfinite(got).all() and (got[0] >= got[1]).all() and (got[1] > 0).all() and (peaks[2 * width:] == 0).all()


# ---- (g) interleaving -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width", [("CS16", 256, 300), ("CU8", 2048, 37)])
def test_execute_and_execute_track_interleave_without_a_synchronisation(ctx, fmt, n, width):
    data, win, bn, _, want = _hop_reference(fmt, n, width, False, n // 2 + 3)
    bands = bandref.standard_bands(n)
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
        plan.execute_track(d_in, data.size, width, bands, out.row, out.peak)
        plan.execute(d_in, data.size, width, *second)
        ctx.synchronize()
        assert_same_reply(reply(first), r_want)
        assert_same_reply(reply(second), r_want)
        trackref.assert_same(out.read("interleaved"), want, "interleaved")
    finally:
        out.free()
        for p_ in first + second + [d_in]:
            ctx.free(p_)
        plan.close()
