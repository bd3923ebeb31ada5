"""The occupancy counts on the GPU (sp_power_occupancy, sp_plan_execute_occupancy, sp_render_occupancy): every comparison is word for
word against tests/occref.py - numpy's >= summed along either axis - on the oracle's plane (tests/powerref.py) or on a synthetic one
with thresholds that plant equality, neighbouring bit patterns, signed zeros, infinities and NaNs.  Every result lies between guard
bytes and holds garbage before the call.

The oracle cases take their thresholds from the oracle's own plane: threshold[y] = K[y] * the row's math.fsum mean (meanref), where K
rotates over the rows through K_ROTATION.  One K for all rows cannot give both a row that is never reached (K > 1: the mean is not below
every value) and a row that is always reached (K <= the row's minimum over its mean, below 1), which the telling condition asks for,
so the rotation holds 0 (always reached), factors around 1 (reached in some frames - the capture hops) and 1e6 (never reached).  The
condition is asserted on the expected arrays, before anything is compared.

The measurement that goes with the feature is not asserted here (tools/occupancy_bench.py)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bandref
import meanref
import occref
import powerref
import siggen
import trackref
from __graft_entry__ import ROOT, load_package
from oracle import pyoracle
from test_gpu_parity import _assert_same as assert_same_reply
from test_mean_gpu import FORMATS, GARBAGE, GEN, GUARD, KERNELS, WIDTHS, _capture, _reference, _upload
from test_track_gpu import _hop_reference

pytestmark = pytest.mark.gpu

K_ROTATION = (0.5, 1.0, 2.0, 0.0, 4.0, 1e6, 0.25)
TILE_ROWS = int(re.search(r"#define SP_OCCUPANCY_TILE_ROWS (\d+)", open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()).group(1))


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Out:
    """Two device arrays, uint32 [n] and uint32 [count, width], each between two guards, everything garbage."""

    def __init__(self, ctx, n, count, width):
        self.ctx, self.shapes = ctx, ((n,), (count, width))
        self.sizes = (4 * n, 4 * count * width)
        self.bases = [ctx.alloc(s + 2 * GUARD) for s in self.sizes]
        assert all(b % 8 == 0 for b in self.bases)
        self.rows, self.frames = (b + GUARD for b in self.bases)
        for b, s in zip(self.bases, self.sizes):
            ctx.memset(b, GARBAGE, s + 2 * GUARD)

    def whole(self):
        return [self.ctx.download(b, s + 2 * GUARD) for b, s in zip(self.bases, self.sizes)]

    def read(self, what=""):
        """(rows, frames); the guards of both arrays must be intact."""
        out = []
        for whole, s, shape in zip(self.whole(), self.sizes, self.shapes):
            assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + s:] == GARBAGE).all(), what + ": bytes around the counts were written"
            out.append(whole[GUARD:GUARD + s].view(np.uint32).reshape(shape).copy())
        return tuple(out)

    def free(self):
        for b in self.bases:
            self.ctx.free(b)


def _garbage(a):
    return bool((a.view(np.uint8) == GARBAGE).all())


def _power_occupancy(ctx, plane, thr, bands, what, rows=True, frames=True):
    """sp_power_occupancy of a host plane f64 [width, n] through a device copy; an output that is not asked for stays garbage."""
    width, n = plane.shape
    d_p, d_t, out = _upload(ctx, plane), _upload(ctx, thr), _Out(ctx, n, len(bands), width)
    try:
        ctx.power_occupancy(d_p if width else 0, n, width, d_t, bands, out.rows if rows else 0, out.frames if frames else 0)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_p)
        ctx.free(d_t)
        out.free()


def _execute_occupancy(ctx, plan, d_in, nbytes, width, thr, bands, what):
    d_t, out = _upload(ctx, thr), _Out(ctx, plan.n, len(bands), width)
    try:
        plan.execute_occupancy(d_in, nbytes, width, d_t, bands, out.rows, out.frames)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_t)
        out.free()


# ---- (a) sp_power_occupancy on synthetic planes -------------------------------------------------------------------------------------------
def _most_bands(n):
    """SP_MAX_BANDS bands: empty, one row, everything, the last row, overlapping ones, everything but the end rows (which straddles every
    edge of a load's 64 rows and of a tile), the rows on either side of the tile's edge and of as many 64-row edges as fit - spread over
    all of them -, ragged runs across them, and a band behind the last edge."""
    c = lambda y: max(0, min(n, y))  # noqa: E731
    bands = [(0, 0), (0, 1), (0, n), (n - 1, n), (c(1), c(n - 1)), (0, n // 2 + 1), (n // 4, n), (c(TILE_ROWS - 1), c(TILE_ROWS + 1)),
             (c(TILE_ROWS - 70), c(TILE_ROWS + 70)), (c(TILE_ROWS), n), (c(TILE_ROWS), c(TILE_ROWS)), (c(3), c(3 + 65)), (n, n)]
    edges = list(range(64, n, 64))
    room = bandref.SP_MAX_BANDS - len(bands)
    some = [edges[(k * len(edges)) // room] for k in range(room)] if len(edges) > room else edges
    for k, g in enumerate(some):
        bands.append((c(g - 1), c(g + 1)) if k % 3 else (c(g - 1 - k % 64), c(g + 2 + (5 * k) % 130)))
    while len(bands) < bandref.SP_MAX_BANDS:
        k = len(bands)
        bands.append((c(k % 7), c(k % 7 + k)))
    assert len(bands) == bandref.SP_MAX_BANDS and all(0 <= y0 <= y1 <= n for y0, y1 in bands)
    return bands


@functools.lru_cache(maxsize=None)
def _synthetic(n, width):
    plane = trackref.synthetic_plane(7000 * n + width, n, width)
    thr = occref.planted_thresholds(plane, n + width)
    want = occref.expected(plane, thr, _most_bands(n))
    for a in (plane, thr) + want:
        a.setflags(write=False)
    return plane, thr, want


SHAPES_A = [(n, w) for n in (2, 64, 100, 256) for w in (1, 2, 63, 64, 65, 257)] + [(TILE_ROWS + 100, 9)]


@pytest.mark.parametrize("n,width", SHAPES_A, ids=["n%d-W%d" % s for s in SHAPES_A])
def test_power_occupancy_of_synthetic_planes(ctx, n, width):
    """Planted thresholds (a value of the row itself, its two neighbouring bit patterns, +0.0, -0.0, -1.0, -inf, +inf, three NaNs, the
    smallest denormal, values that differ from a planted one in one half of their bits) against trackref's plane (ties, NaNs of three
    kinds, infinities, all +0.0, DBL_MAX, denormals), with 64 bands.  n = 100 is no multiple of a load's 64 rows, widths 1 and 2 are less
    than a workgroup's frames, 63, 65 and 257 no multiple of them, 64 is one; the last shape spans two row tiles."""
    plane, thr, want = _synthetic(n, width)
    bands = _most_bands(n)
    what = "sp_power_occupancy n=%d W=%d" % (n, width)
    assert n <= TILE_ROWS or any(y0 < TILE_ROWS < y1 and want[1][b].any() for b, (y0, y1) in enumerate(bands))
    both = _power_occupancy(ctx, plane, thr, bands, what)
    occref.assert_same(both, want, what)
    assert not both[1][0].any() and not both[1][12].any()                                       # the empty bands
    assert np.array_equal(both[1][2].astype(np.int64).sum(), both[0].astype(np.int64).sum())    # the full band holds every hit
    # either output alone: the same words, the other one untouched, the guards intact
    only_rows = _power_occupancy(ctx, plane, thr, bands, what + " rows only", frames=False)
    assert np.array_equal(only_rows[0], both[0]) and _garbage(only_rows[1])
    only_frames = _power_occupancy(ctx, plane, thr, bands, what + " frames only", rows=False)
    assert np.array_equal(only_frames[1], both[1]) and _garbage(only_frames[0])
    # rows without any band
    no_bands = _power_occupancy(ctx, plane, thr, [], what + " no bands")
    assert np.array_equal(no_bands[0], both[0])


def test_power_occupancy_of_the_standard_bands_and_scalar_thresholds(ctx):
    n, width = 100, 65
    plane = _synthetic(n, width)[0]
    bands = bandref.standard_bands(n)
    for value in (0.0, 0.5, 2.0, np.inf, -np.inf, np.nan):
        thr = np.full(n, value)
        what = "threshold %r" % value
        occref.assert_same(_power_occupancy(ctx, plane, thr, bands, what), occref.expected(plane, thr, bands), what)


# ---- (b) sp_plan_execute_occupancy against the oracle's plane -------------------------------------------------------------------------------
ORACLE_KERNELS = [1, 2, 5, 4]      # of test_mean_gpu.KERNELS: frames_power at n = 256 and 1024, scratch_power forced at 256 and at 2048


def _thresholds_of(plane, mean):
    k = np.array([K_ROTATION[y % len(K_ROTATION)] for y in range(plane.shape[1])])
    thr = k * np.asarray(mean, np.float64)      # (one IEEE multiply per row)
    thr[np.isnan(thr)] = np.inf                 # (a row whose mean is no number - channel mode's row 0 - is never reached)
    return thr


def _assert_telling(plane, thr, want, what, moving=True):
    """The condition on the inputs: the expected counts alone must tell a wrong compare, a lost frame or a lost row from a right one."""
    rows, frames = want
    width, n = plane.shape
    share = int(rows.astype(np.int64).sum()) / float(width * n)
    assert 0.02 <= share <= 0.98, "%s: %.3f of all values are hits" % (what, share)
    assert (rows == 0).any() and (rows == width).any(), what + ": no row without a hit, or none with every frame"
    if moving:
        assert len(np.unique(frames[2])) >= 8, what + ": the full band's count takes fewer than 8 values"


@functools.lru_cache(maxsize=None)
def _oracle_case(fmt, n, width, ch, stride):
    """(capture, taper, block_norm, plane, thresholds, expected of bandref.standard_bands(n)) on test_track_gpu's hopping capture: the
    plane is that module's, computed once for both."""
    data, win, bn, plane, _ = _hop_reference(fmt, n, width, ch, stride)
    thr = _thresholds_of(plane, meanref.expected(plane))      # (math.fsum per row, divided by the width)
    want = occref.expected(plane, thr, bandref.standard_bands(n))
    _assert_telling(plane, thr, want, "%s n=%d W=%d" % (fmt, n, width), moving=width >= 37)
    for a in (thr,) + want:
        a.setflags(write=False)
    return data, win, bn, plane, thr, want


@pytest.mark.parametrize("k", ORACLE_KERNELS, ids=["n%d%s" % (KERNELS[k][0], "-forced" if KERNELS[k][1] else "") for k in ORACLE_KERNELS])
@pytest.mark.parametrize("j", range(len(WIDTHS)), ids=["W%d" % w for w in WIDTHS])
def test_execute_occupancy_against_the_oracle(ctx, k, j):
    """frames_power at n = 256 and 1024, scratch_power at n = 256 (forced) and 2048, at every width of the track's oracle test on its
    hopping capture; the format and the channel mode rotate as there."""
    n, forced, name = KERNELS[k]
    width = WIDTHS[j]
    fmt, ch = FORMATS[(k + j) % 3], (k // 3 + j) % 2 == 1
    data, win, bn, plane, thr, want = _oracle_case(fmt, n, width, ch, n // 2 + 3)
    what = "%s n=%d W=%d%s%s" % (fmt, n, width, " L/R" if ch else "", " forced" if forced else "")
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.occupancy_kernel_name_for(data.size, width) == name + "+occupancy"
        got = _execute_occupancy(ctx, plan, d_in, data.size, width, thr, bandref.standard_bands(n), what)
    finally:
        ctx.free(d_in)
        plan.close()
    occref.assert_same(got, want, what)


def test_kernel_name_both_ways(ctx):
    for n, name in ((256, "frames_power+occupancy"), (2048, "scratch_power+occupancy")):
        win, weight = pyoracle.window("hann", n)
        plan = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
        try:
            assert plan.occupancy_kernel_name_for(4 * 40 * n, 37) == name
            plan.force_kernel("scratch")
            assert plan.occupancy_kernel_name_for(4 * 40 * n, 37) == "scratch_power+occupancy"
        finally:
            plan.close()
    assert ctx.lib.L.sp_plan_occupancy_kernel_name_for(None, 0, 0) == b""


# ---- (c) order-freedom ------------------------------------------------------------------------------------------------------------------------
SHAPES = [("CS16", 256, 300, False), ("CF32", 1024, 37, True), ("CU8", 2048, 37, False)]


@pytest.mark.parametrize("fmt,n,width,ch", SHAPES)
def test_the_window_does_not_change_a_word(ctx, fmt, n, width, ch):
    data, win, bn, _, thr, want = _oracle_case(fmt, n, width, ch, n // 2 + 3)
    bands = bandref.standard_bands(n)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    got = []
    try:
        for window in (8 * n, 3 * 8 * n, 1, 0):        # one frame, three frames, below one frame (one frame), the default
            ctx.set_mean_window(window)
            got.append(_execute_occupancy(ctx, plan, d_in, data.size, width, thr, bands, "window %d" % window))
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()
    for g in got:
        occref.assert_same(g, want, "window")


@pytest.mark.parametrize("fmt,n,width,ch", SHAPES)
def test_counts_of_the_plane_are_the_counts_of_the_request(ctx, fmt, n, width, ch):
    data, win, bn, _, thr, want = _oracle_case(fmt, n, width, ch, n // 2 + 3)
    bands = bandref.standard_bands(n)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    d_in, d_plane, d_t = _upload(ctx, data), ctx.alloc(8 * width * n), _upload(ctx, thr)
    direct, from_plane = _Out(ctx, n, len(bands), width), _Out(ctx, n, len(bands), width)
    try:
        plan.execute_occupancy(d_in, data.size, width, d_t, bands, direct.rows, direct.frames)
        plan.execute_power(d_in, data.size, width, d_plane)
        ctx.power_occupancy(d_plane, n, width, d_t, bands, from_plane.rows, from_plane.frames)
        ctx.synchronize()
        got, got_plane = direct.read("direct"), from_plane.read("from the plane")
    finally:
        for p in (d_in, d_plane, d_t):
            ctx.free(p)
        for o in (direct, from_plane):
            o.free()
        plan.close()
    occref.assert_same(got, want, "sp_plan_execute_occupancy")
    occref.assert_same(got_plane, want, "sp_power_occupancy of sp_plan_execute_power's plane")
    # ... and the host entry gives the same words, with a scalar threshold too
    occref.assert_same(ctx.render_occupancy(fmt, data, n, win, bn, 3.0, 50.0, width, thr, bands, ch, fill=GARBAGE), want, "Context.render_occupancy")


# ---- (d) the host entry point -------------------------------------------------------------------------------------------------------------------
def _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, thr, bands, ch=False, rows=True, frames=True):
    """sp_render_occupancy into two host arrays between guards, everything garbage: (status, (rows, frames), the guards are intact)."""
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, ch, False)
    b = np.ascontiguousarray(np.asarray(bands, np.int32).reshape(-1, 2))
    thr = np.ascontiguousarray(thr, np.float64)
    count, w = b.shape[0], max(width, 0)
    hosts = [np.full(s + 2 * GUARD, GARBAGE, np.uint8) for s in (4 * n, 4 * count * w)]
    vp = C.c_void_p
    rc = ctx.lib.L.sp_render_occupancy(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, width, thr.ctypes.data_as(vp),
                                       b.ctypes.data_as(vp) if count else None, count, vp(hosts[0].ctypes.data + GUARD) if rows else None,
                                       vp(hosts[1].ctypes.data + GUARD) if frames else None)
    intact = all(bool((h[:GUARD] == GARBAGE).all() and (h[h.size - GUARD:] == GARBAGE).all()) for h in hosts)
    got_rows = hosts[0][GUARD:hosts[0].size - GUARD].view(np.uint32).copy()
    got_frames = hosts[1][GUARD:hosts[1].size - GUARD].view(np.uint32).reshape(count, w).copy()
    return rc, (got_rows, got_frames), intact


def test_small_sparse_request_uploads_its_frames_only(pkg, ctx):
    fmt, n, width = "CU8", 256, 64
    data, win, bn, plane, thr, want = _oracle_case(fmt, n, width, False, 40 * n + 11)
    bands = bandref.standard_bands(n)
    rc, got, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, thr, bands)
    assert rc == 0 and intact
    occref.assert_same(got, want, "sparse sp_render_occupancy")
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1
    # either output alone: the other array stays garbage
    rc, only_rows, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, thr, bands, frames=False)
    assert rc == 0 and intact and np.array_equal(only_rows[0], want[0]) and _garbage(only_rows[1])
    rc, only_frames, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, thr, bands, rows=False)
    assert rc == 0 and intact and np.array_equal(only_frames[1], want[1]) and _garbage(only_frames[0])
    # a scalar threshold is every row's
    value = float(np.median(plane))
    got = ctx.render_occupancy(fmt, data, n, win, bn, 3.0, 50.0, width, value, bands, fill=GARBAGE)
    occref.assert_same(got, occref.expected(plane, np.full(n, value), bands), "Context.render_occupancy with a scalar threshold")
    with pytest.raises(ValueError):
        ctx.render_occupancy(fmt, data, n, win, bn, 3.0, 50.0, width, thr[:-1], bands)


def test_chunked_sp_render_occupancy(pkg, ctx):
    """stride n, 16 MiB - the smallest request the streamer cuts: the capture travels in chunks and every chunk adds its hits.  (The
    plane and its mean are the mean test's, computed once for all.)"""
    fmt, n, width = "CF32", 1024, 2048
    data, win, bn, plane, mean = _reference(fmt, n, width, False, n)
    bands = bandref.standard_bands(n)
    thr = _thresholds_of(plane, mean)
    want = occref.expected(plane, thr, bands)
    _assert_telling(plane, thr, want, "chunked", moving=False)
    assert data.size >= 16 << 20
    rc, got, intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, thr, bands)
    assert rc == 0 and intact
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    occref.assert_same(got, want, "chunked sp_render_occupancy")


@pytest.mark.parametrize("n", [64, 2048])
def test_capture_shorter_than_n_gives_zeros_everywhere(pkg, ctx, n):
    data = siggen.generate("CS16", GEN, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    thr = np.array([(0.0, -np.inf, 1.0, -1.0)[y % 4] for y in range(n)])
    rc, (rows, frames), intact = _render_guarded(ctx, pkg, "CS16", data, n, win, 1.0 / weight, 3, thr, [(0, n), (1, 2), (n - 1, n), (5, 5)])
    assert rc == 0 and intact and rows.shape == (n,) and frames.shape == (4, 3) and not rows.any() and not frames.any()


def test_width_0_and_count_0(pkg, ctx):
    """width == 0: `rows` all zero, `frames` untouched; count == 0: `rows` as with bands, `frames` untouched."""
    fmt, n, width = "CU8", 256, 64
    data, win, bn, _, thr, want = _oracle_case(fmt, n, width, False, 40 * n + 11)
    rc, (rows, frames), intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, 0, thr, [(0, n), (3, 9)])
    assert rc == 0 and intact and not rows.any() and frames.size == 0
    rc, (rows, frames), intact = _render_guarded(ctx, pkg, fmt, data, n, win, bn, width, thr, [])
    assert rc == 0 and intact and np.array_equal(rows, want[0]) and frames.size == 0
    # a frames array alone that nothing is written to: SP_OK and untouched
    host = np.full(2 * GUARD, GARBAGE, np.uint8)
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, bn, 3.0, 50.0, powerref._LUT, False, False)
    vp = C.c_void_p
    b = np.array([[0, n]], np.int32)
    rt = ctx.lib.L.sp_render_occupancy
    assert rt(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, 0, thr.ctypes.data_as(vp), b.ctypes.data_as(vp), 1, None,
              vp(host.ctypes.data + GUARD)) == 0
    assert rt(ctx.h, C.byref(req), data.ctypes.data_as(vp), data.size, width, thr.ctypes.data_as(vp), None, 0, None,
              vp(host.ctypes.data + GUARD)) == 0
    assert (host == GARBAGE).all()
    # the device entries
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in, d_plane, d_t = _upload(ctx, data), ctx.alloc(8 * width * n), _upload(ctx, thr)
    outs = [_Out(ctx, n, 1, 1) for _ in range(5)]
    try:
        plan.execute_occupancy(d_in, data.size, 0, d_t, [(0, n)], outs[0].rows, outs[0].frames)
        plan.execute_occupancy(d_in, data.size, width, d_t, [], outs[1].rows, outs[1].frames)
        ctx.power_occupancy(d_plane, n, 0, d_t, [(0, n)], outs[2].rows, outs[2].frames)
        ctx.power_occupancy(0, n, 0, d_t, [(0, n)], outs[3].rows, outs[3].frames)
        plan.execute_occupancy(d_in, data.size, 0, d_t, [(0, n)], 0, outs[4].frames)
        plan.execute_occupancy(d_in, data.size, width, d_t, [], 0, outs[4].frames)
        ctx.power_occupancy(0, n, 0, d_t, [(0, n)], 0, outs[4].frames)
        ctx.synchronize()
        for k, o in enumerate(outs[:4]):
            rows, frames = o.read("case %d" % k)
            assert _garbage(frames), k
            assert np.array_equal(rows, want[0]) if k == 1 else not rows.any(), k
        assert all((w == GARBAGE).all() for w in outs[4].whole())
    finally:
        for o in outs:
            o.free()
        for p in (d_in, d_plane, d_t):
            ctx.free(p)
        plan.close()


# ---- (e) refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    d_in, d_plane, d_t = ctx.alloc(data.size), ctx.alloc(8 * width * n + 16), ctx.alloc(8 * n + 16)
    out = _Out(ctx, n + 4, 64, width + 1)
    d_rows, d_frames = out.rows, out.frames
    vp = C.c_void_p

    def arr(*rows):
        return (C.c_int32 * len(rows))(*rows)

    ok, many = arr(0, n, 3, 9), arr(*([0, 1] * 65))
    bad_bands = [(arr(0, n + 1), 1), (arr(-1, 4), 1), (arr(5, 4), 1), (arr(0, n, n + 1, n + 1), 2), (many, 65), (ok, -1), (None, 1)]
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_occupancy(d_in, data.size, width, d_t, [(0, n)], d_rows, d_frames)
        assert e.value.status == -4 and "peak" in str(e.value)
        ex = L.sp_plan_execute_occupancy
        po = L.sp_power_occupancy
        assert ex(None, vp(d_in), data.size, width, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        for bands, count in bad_bands:
            assert ex(plan.h, vp(d_in), data.size, width, vp(d_t), bands, count, vp(d_rows), vp(d_frames)) == -1, count
            assert po(ctx.h, vp(d_plane), n, width, vp(d_t), bands, count, vp(d_rows), vp(d_frames)) == -1, count
        for f in (lambda *a: ex(plan.h, vp(d_in), data.size, width, *a), lambda *a: po(ctx.h, vp(d_plane), n, width, *a)):
            assert f(None, ok, 2, vp(d_rows), vp(d_frames)) == -1                       # no thresholds
            assert f(vp(d_t + 4), ok, 2, vp(d_rows), vp(d_frames)) == -1                # misaligned thresholds
            assert f(vp(d_t), ok, 2, vp(d_rows + 2), vp(d_frames)) == -1                # misaligned rows
            assert f(vp(d_t), ok, 2, vp(d_rows), vp(d_frames + 2)) == -1                # misaligned frames
            assert f(vp(d_t), ok, 2, None, None) == -1                                  # both NULL
            assert f(vp(d_t), None, 0, None, None) == -1
        assert ex(plan.h, vp(d_in), data.size, -1, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        assert ex(plan.h, None, data.size, width, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        plan16 = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
        assert ex(plan16.h, vp(d_in), 4 * 100 + 1, width, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -3
        plan16.close()
        assert po(None, vp(d_plane), n, width, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        assert po(ctx.h, vp(d_plane), 0, width, vp(d_t), arr(0, 0), 1, vp(d_rows), vp(d_frames)) == -1
        assert po(ctx.h, vp(d_plane), (1 << 20) + 1, 0, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        assert po(ctx.h, vp(d_plane), n, -1, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        assert po(ctx.h, vp(d_plane + 4), n, width, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        assert po(ctx.h, None, n, width, vp(d_t), ok, 2, vp(d_rows), vp(d_frames)) == -1
        assert po(ctx.h, vp(d_plane), 100, width, vp(d_t), arr(0, 101), 1, vp(d_rows), vp(d_frames)) == -1      # any n >= 1: its own bound
        ctx.synchronize()
        rows, frames = out.read("refusals")
        assert _garbage(rows) and _garbage(frames)           # nothing was written by any of them
        # ... and what is allowed
        ctx.memset(d_t, 0, 8 * n + 16)                       # thresholds of +0.0: every value that is a number hits
        assert ex(plan.h, vp(d_in), data.size, width, vp(d_t), many, 64, vp(d_rows), vp(d_frames)) == 0           # 64 bands
        assert ex(plan.h, vp(d_in), data.size, width, vp(d_t + 8), ok, 2, vp(d_rows + 4), vp(d_frames + 4)) == 0  # 8 and 4 bytes are enough
        assert ex(plan.h, vp(d_in), data.size, width, vp(d_t), ok, 2, vp(d_rows), None) == 0                      # either one may be NULL
        assert ex(plan.h, vp(d_in), data.size, width, vp(d_t), ok, 2, None, vp(d_frames)) == 0
        assert ex(plan.h, vp(d_in), data.size, width, vp(d_t), None, 0, vp(d_rows), None) == 0                    # rows need no bands
        ctx.synchronize()
        out.read("allowed")
    finally:
        peak.close()
        plan.close()
        out.free()
        for p_ in (d_in, d_plane, d_t):
            ctx.free(p_)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "peak")
    rows, frames, thr = np.full(n, 7, np.uint32), np.full(64 * width, 7, np.uint32), np.zeros(n + 1)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    rt = L.sp_render_occupancy
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, p(thr), ok, 2, p(rows), p(frames)) == -4
    req.detector = 0
    assert rt(None, C.byref(req), p(data), data.size, width, p(thr), ok, 2, p(rows), p(frames)) == -1
    assert rt(ctx.h, None, p(data), data.size, width, p(thr), ok, 2, p(rows), p(frames)) == -1
    assert rt(ctx.h, C.byref(req), None, data.size, width, p(thr), ok, 2, p(rows), p(frames)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, -2, p(thr), ok, 2, p(rows), p(frames)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, None, ok, 2, p(rows), p(frames)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, vp(thr.ctypes.data + 4), ok, 2, p(rows), p(frames)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, p(thr), ok, 2, None, None) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, p(thr), ok, 2, vp(rows.ctypes.data + 2), p(frames)) == -1
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, p(thr), ok, 2, p(rows), vp(frames.ctypes.data + 1)) == -1
    for bands, count in bad_bands:
        assert rt(ctx.h, C.byref(req), p(data), data.size, width, p(thr), bands, count, p(rows), p(frames)) == -1, count
    req16, keep16 = pkg.binding._make_request(pkg.parse_format("CS16")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False)
    assert rt(ctx.h, C.byref(req16), p(data), 4 * 100 + 1, width, p(thr), ok, 2, p(rows), p(frames)) == -3
    assert (rows == 7).all() and (frames == 7).all()
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, vp(thr.ctypes.data + 8), ok, 2, p(rows), None) == 0        # the rows alone
    assert (rows == width).all() and (frames == 7).all()                                                           # every value >= +0.0
    assert rt(ctx.h, C.byref(req), p(data), data.size, width, p(thr), ok, 2, p(rows), p(frames)) == 0
    assert (frames[:width] == n).all() and (frames[width:2 * width] == 6).all() and (frames[2 * width:] == 7).all()


# ---- (f) interleaving -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width", [("CS16", 256, 300), ("CU8", 2048, 37)])
def test_execute_track_and_occupancy_interleave_without_a_synchronisation(ctx, fmt, n, width):
    data, win, bn, plane, thr, want = _oracle_case(fmt, n, width, False, n // 2 + 3)
    t_want = _hop_reference(fmt, n, width, False, n // 2 + 3)[4]
    bands = bandref.standard_bands(n)
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    r_want = pyoracle.render(fmt, data, n, win, bn, 3.0, 50.0, lut, width)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, lut)
    d_in, d_t = _upload(ctx, data), _upload(ctx, thr)
    sizes = [4 * width * n, width, width, width, 8 * 256, 8000, 16]
    first = [ctx.alloc(s_) for s_ in sizes]
    second = [ctx.alloc(s_) for s_ in sizes]
    out, again = _Out(ctx, n, len(bands), width), _Out(ctx, n, len(bands), width)
    d_row, d_peak = ctx.alloc(4 * len(bands) * width), ctx.alloc(8 * len(bands) * width)

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
        plan.execute_occupancy(d_in, data.size, width, d_t, bands, out.rows, out.frames)
        plan.execute_track(d_in, data.size, width, bands, d_row, d_peak)
        plan.execute_occupancy(d_in, data.size, width, d_t, bands, again.rows, again.frames)
        plan.execute(d_in, data.size, width, *second)
        ctx.synchronize()
        assert_same_reply(reply(first), r_want)
        assert_same_reply(reply(second), r_want)
        occref.assert_same(out.read("interleaved"), want, "interleaved")
        occref.assert_same(again.read("interleaved again"), want, "interleaved again")
        t_got = (ctx.download(d_row, 4 * len(bands) * width, np.int32).reshape(len(bands), width),
                 ctx.download(d_peak, 8 * len(bands) * width, np.float64).reshape(len(bands), width))
        trackref.assert_same(t_got, t_want, "the track between them")
    finally:
        out.free()
        again.free()
        for p_ in first + second + [d_in, d_t, d_row, d_peak]:
            ctx.free(p_)
        plan.close()
