"""Whole-reply parity of the portable ("scratch") kernels where a workgroup serves more than one column, where the four-stage frame ends
in a group of three stages, and up to n = SP_MAX_N.

Each case is ONE launch on device-resident operands whose shape - workgroups, four-stage variant - is computed with tests/scratchref.py
for the CU count of the part the test runs on (read from sp_plan_debug_launch), confirmed through sp_debug_scratch_launch and the
kernel_name*() entries before anything is rendered, and compared whole and bit for bit: the image replies with the oracle
(pyoracle.render), the peak plan's with peakref.expected, the traces with tracesref.expected, the power plane with powerref.expected.
No tolerance.  Inputs are trinoise; the image and peak captures hold three zeroed frames, one of them a later column of its workgroup;
the LUT is injective; every output starts as garbage and lies between guard bytes that must survive.  B = scratchref.workgroups(...).

B1  several columns per workgroup at moderate n: widths of B + c, 2 B + c, 3 B + c frames.
B2  n = 2^15 (the first frame whose last barrier group has three stages), 2^19 (three stages behind four full groups), 2^20
    (SP_MAX_N): three frames each.
B3  the 256 MiB of slabs as the bound of the workgroups: 16 or 10 of them, one frame or three more than twice or once that.
B4  every consumer of the power plane and of the index image at n = SP_MAX_N against its reference module; sp_power_* at a row
    count that is no power of two; a request at 2 n refused.
The last test asserts that every case ran."""
import functools

import numpy as np
import pytest

import bandref
import burstref
import densityref
import meanref
import occref
import peakref
import powerref
import pulseref
import quantileref
import scratchref
import siggen
import test_index_launch_shapes_gpu as shapes
import test_launch_shapes_gpu as base
import tracesref
import trackref
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GAIN, RANGE, GUARD = base.GAIN, base.RANGE, 4096
MAX_N = scratchref.MAX_N
pkg, ctx, cu = base.pkg, base.ctx, base.cu   # (module-scoped fixtures, instantiated for this module)


def _case(part, kind, n, fmt, ch=False, wf=False, k=0, plus=3, hop=None, M=1, oob=False, force=False):
    """Width = k * B + plus frames (k = 0: a fixed width).  hop: whole samples between two frames (a fraction is added); a peak case's
    stride follows from M."""
    c = dict(part=part, kind=kind, n=n, fmt=fmt, ch=ch, wf=wf, k=k, plus=plus, hop=hop if hop else n // 8, M=M, oob=oob, force=force)
    c["id"] = "%s_%s_n%d_%s%s%s%s%s_%s" % (part, kind, n, fmt, "_lr" if ch else "", "_wf" if wf else "", "_M%d" % M if M > 1 else "",
                                           "_oob" if oob else "", "%dB+%d" % (k, plus) if k else "W%d" % plus)
    return c


def _b2():
    """At each n an image, a peak, a traces and a power case of three frames; formats and layouts rotate, both channel modes occur at
    n = 2^20, the 2^19 image request ends past its capture."""
    out = []
    for i, n in enumerate((1 << 15, 1 << 19, 1 << 20)):
        for j, kind in enumerate(("image", "peak", "traces", "power")):
            out.append(_case("B2", kind, n, ("CF32", "CS12", "CU8")[(i + j) % 3], ch=(i + j) % 2 == 1, wf=kind in ("image", "peak") and (i + j // 2) % 2 == 0,
                             plus=3, hop=n // 2 + 3, M=2 if kind == "peak" else 1, oob=kind == "image" and n == 1 << 19))
    # the two smaller groups that can end a four-stage frame: one stage at n = 8192, two at n = 16384
    out.append(_case("B2", "image", 8192, "CS16", wf=True, plus=3, hop=8192 // 2 + 3, force=True))
    out.append(_case("B2", "power", 16384, "CF32", ch=True, plus=3, hop=16384 // 2 + 3))
    return out


CASES = [
    _case("B1", "image", 32, "CS16", wf=True, k=2, plus=5),
    _case("B1", "image", 4096, "CU8", ch=True, k=2, plus=7, force=True),
    _case("B1", "image", 4096, "CF32", k=1, plus=3, oob=True, force=True),
    _case("B1", "peak", 32, "CS8", k=1, plus=5, M=3),
    _case("B1", "peak", 4096, "CS16", wf=True, k=1, plus=5, M=2, force=True),
    _case("B1", "traces", 2048, "CU8", k=3, plus=5, hop=262),
    _case("B1", "traces", 4096, "CS16", k=3, plus=5, hop=515),
    _case("B1", "power", 2048, "CS12", k=2, plus=5),
    _case("B1", "power", 4096, "CF32", ch=True, k=1, plus=9),
] + _b2() + [
    _case("B3", "image", 1 << 20, "CU8", k=1, plus=3, hop=1 << 17),
    _case("B3", "traces", 1 << 19, "CS16", k=2, plus=3, hop=1 << 16),
    _case("B3", "peak", 1 << 20, "CU8", k=1, plus=1, M=2),
]
CONSUMERS = ("index", "density", "mean", "mean_one_frame", "bandpower", "track", "occupancy", "quantile", "quantile_one_frame", "bursts", "pulses",
             "any_n", "refused")
RAN = set()


def last_groups():
    """The sizes of the last barrier group among the cases that run the four-stage variant."""
    return {scratchref.stage_groups(c["n"].bit_length() - 1)[-1] for c in CASES if scratchref.wide(c["n"])}


def _shape(c, cu):
    """(W, B) of a case on a part of cu CUs."""
    slabs = scratchref.SLABS[c["kind"]]
    if not c["k"]:
        return c["plus"], scratchref.workgroups(c["n"], slabs, c["plus"], cu)
    B = scratchref.workgroups(c["n"], slabs, 1 << 30, cu)
    W = c["k"] * B + c["plus"]
    assert scratchref.workgroups(c["n"], slabs, W, cu) == B < W
    return W, B


def _silenced(W, B):
    """The frames that hold zeros: the second, a middle one, and one that is a later column of its workgroup where there is one."""
    return sorted({1, W // 2, max(W - 2, B) if W > B else W - 2} & set(range(W)))


def _capture(c, W, B):
    n, fmt, M = c["n"], c["fmt"], c["M"]
    sw = siggen.SAMPLE_WIDTH[fmt]
    samples = n + (W - 1) * M * n + (W - 1) // 2 + 1 if M > 1 else n + (W - 1) * c["hop"] + (W - 1) // 3 + 1
    data = base._trinoise(fmt, samples, seed=n.bit_length())
    if c["oob"]:
        e = base.ELEM[fmt]
        data = np.concatenate([data, np.full(e * -(-sw // (2 * e)), 0x5A, np.uint8)])
    if c["kind"] in ("image", "peak"):   # (a zero would be every bin's minimum in a trace and a repeated value in a plane)
        xs = _silenced(W, B)
        assert W <= B or max(xs) >= B
        for x in xs:
            s = base._start(data.size / sw, n, W, x)
            data[s * sw:(s + n) * sw] = 0
    return data


def _telling_traces(want, W, B, what):
    """A held minimum or maximum that is lost, or one that is sent before the workgroup's last column, cannot hide: the extremes of many
    bins lie in a later column of their workgroup, and those of many others in its first."""
    n = len(want["min_column"])
    for key in ("min_column", "max_column"):
        later = int((want[key] >= B).sum())
        assert 4 * later >= n and 8 * (n - later) >= n, "%s: %s: %d of %d bins in a column >= %d" % (what, key, later, n, B)


def _make(c, cu):
    """The capture and the reference of a case."""
    W, B = _shape(c, cu)
    n, fmt = c["n"], c["fmt"]
    data = _capture(c, W, B)
    win, weight = pyoracle.window("blackmanHarris" if c["wf"] else "hann", n)
    bn = 1.0 / weight
    what = "%s W=%d B=%d" % (c["id"], W, B)
    if c["kind"] == "image":
        want = pyoracle.render(fmt, data, n, win, bn, GAIN, RANGE, base._lut(), W, c["ch"], c["wf"])
    elif c["kind"] == "peak":
        want = peakref.expected(fmt, data, n, win, bn, GAIN, RANGE, base._lut(), W, c["ch"], c["wf"])
        assert want["M"] == c["M"] and want["counts"][-1] < c["M"] and all(v == c["M"] for v in want["counts"][:-1]), what
        for key in ("jstar", "counts"):
            want.pop(key)
    elif c["kind"] == "traces":
        want = tracesref.expected(fmt, data, n, win, bn, GAIN, RANGE, W, c["ch"], columns=W > B)
        if W > B:
            _telling_traces(want, W, B, what)
    else:
        want = powerref.expected(fmt, data, n, win, bn, GAIN, RANGE, W, c["ch"])["power"]
        powerref.assert_telling(want[:, 1:] if c["ch"] else want, what)      # (row 0 of an L/R split is bin n / 2: zero)
    return W, B, data, win, bn, want, what


@pytest.fixture(scope="module")
def ahead(cu):
    pyoracle.lib()
    a = base._Ahead(CASES, lambda c: _make(c, cu), depth=3)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


class _Dev:
    """`nbytes` of device memory between two guards, everything garbage."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.base = ctx.alloc(nbytes + 2 * GUARD)
        assert self.base % 16 == 0
        self.ptr = self.base + GUARD
        ctx.memset(self.base, 0xAB, nbytes + 2 * GUARD)

    def read(self, dtype, what):
        whole = self.ctx.download(self.base, self.nbytes + 2 * GUARD)
        assert (whole[:GUARD] == 0xAB).all() and (whole[GUARD + self.nbytes:] == 0xAB).all(), what + ": bytes around an output were written"
        return whole[GUARD:GUARD + self.nbytes].view(dtype)

    def free(self):
        self.ctx.free(self.base)


def _assert_shape(pkg, c, cu, W, B, what):
    """The launch of the case through the library's own functions: its workgroups and its variant; more columns than workgroups where
    the case is about a workgroup's later columns; the cap, not the part, as the bound where the case is about the cap."""
    n, slabs = c["n"], scratchref.SLABS[c["kind"]]
    got = pkg.binding.debug_scratch_launch(n, slabs, W, cu)
    assert got == (B, scratchref.wide(n)) == (scratchref.workgroups(n, slabs, W, cu), n >= 4096), (what, got)
    assert len(scratchref.columns_of(0, W, B)) == -(-W // B) and sum(len(scratchref.columns_of(b, W, B)) for b in range(B)) == W
    if c["part"] in ("B1", "B3"):
        assert B < W and len(scratchref.columns_of(0, W, B)) >= 2, what
    if c["part"] == "B3":
        assert B == scratchref.CAP_BYTES // (8 * slabs * n) < 4 * cu, what
    if c["part"] == "B2":
        assert B == W == 3 and scratchref.stage_groups(n.bit_length() - 1)[-1] == {13: 1, 14: 2, 15: 3, 19: 3, 20: 4}[n.bit_length() - 1], what


def run_case(pkg, ctx, cu, c, made):
    """One case - its capture and reference are `made` = _make(c, cu) - through its one launch, the shape confirmed first."""
    n, kind = c["n"], c["kind"]
    W, B, data, win, bn, want, what = made
    lut = base._lut()
    plan = ctx.plan(c["fmt"], n, win, bn, GAIN, RANGE, lut, c["ch"], c["wf"], detector="peak" if kind == "peak" else "sample")
    d_in = ctx.alloc(data.size + 16)
    try:
        if c["force"]:
            plan.force_kernel("scratch")
        _assert_shape(pkg, c, cu, W, B, what)
        ctx.upload(d_in, data)
        if kind in ("image", "peak"):
            assert plan.kernel_name(data.size, W) == "scratch_radix2", what
            ptrs, blk = base._alloc_reply(ctx, W, n, len(lut), False)
            try:
                d = plan.debug_launch(data.size, W, ptrs["rgba"])
                assert d["kernel"] == "scratch_radix2" and d["cu_count"] == cu and d["peak_m"] == c["M"] and d["log2n"] == n.bit_length() - 1, (what, d)
                plan.execute(d_in, data.size, W, **ptrs)
                ctx.synchronize()
                got = base._read_reply(ctx, ptrs, blk, W, n, len(lut), what)
            finally:
                base._free_reply(ctx, ptrs, blk)
            base._same(got, want, what)
        elif kind == "traces":
            assert plan.traces_kernel_name_for(data.size, W) == "scratch_traces", what
            lo, hi = _Dev(ctx, 8 * n), _Dev(ctx, 8 * n)
            try:
                plan.execute_traces(d_in, data.size, W, lo.ptr, hi.ptr)
                ctx.synchronize()
                got = {"trace_min": lo.read(np.float64, what), "trace_max": hi.read(np.float64, what)}
            finally:
                lo.free()
                hi.free()
            tracesref.assert_same(got, want, what)
        else:
            assert plan.power_kernel_name_for(data.size, W) == "scratch_power", what
            pl = _Dev(ctx, 8 * W * n)
            try:
                plan.execute_power(d_in, data.size, W, pl.ptr)
                ctx.synchronize()
                got = pl.read(np.float64, what).reshape(W, n)
            finally:
                pl.free()
            powerref.assert_same(got, want, what)
    finally:
        ctx.free(d_in)
        plan.close()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["id"] for c in CASES])
def test_scratch_whole_reply(pkg, ctx, cu, ahead, k):
    run_case(pkg, ctx, cu, CASES[k], ahead.get(k))
    RAN.add(CASES[k]["id"])


# ------------------------------------------------------------------------------------------------------ B4: the consumers at SP_MAX_N
FMT4, W4 = "CS12", 3


@functools.lru_cache(maxsize=None)
def _max_n():
    """The request every consumer gets: (capture, taper, block_norm, the oracle's plane f64 [3, 2^20] in row order), read-only."""
    n = MAX_N
    data = base._trinoise(FMT4, n + (W4 - 1) * (n // 2 + 3) + 1, seed=4)
    win, weight = pyoracle.window("hann", n)
    plane = powerref.expected(FMT4, data, n, win, 1.0 / weight, GAIN, RANGE, W4)["power"]
    powerref.assert_telling(plane, "the plane at SP_MAX_N")
    for a in (data, win, plane):
        a.setflags(write=False)
    return data, win, 1.0 / weight, plane


@functools.lru_cache(maxsize=None)
def _band_series():
    """(bands, their exact sums over the plane, hi, lo: the thresholds from every series' own median, as test_bursts_gpu takes them)"""
    bands = bandref.standard_bands(MAX_N)
    sums = bandref.expected(_max_n()[3], bands)
    median = np.sort(sums, axis=1)[:, (W4 - 1) // 2]
    return bands, sums, 4.0 * median, 2.0 * median


@pytest.fixture(scope="module")
def rig(pkg, ctx, cu):
    """The capture on the device and a plan for it; the launch behind every consumer is the power plane's (or the image's) of B2."""
    data, win, bn, _ = _max_n()
    assert pkg.binding.debug_scratch_launch(MAX_N, 2, W4, cu) == (3, True) == (scratchref.workgroups(MAX_N, 2, W4, cu), scratchref.wide(MAX_N))
    plan = ctx.plan(FMT4, MAX_N, win, bn, GAIN, RANGE, base._lut())
    d_in = ctx.alloc(data.size + 16)
    ctx.upload(d_in, data)
    yield plan, d_in, data.size
    ctx.set_mean_window(0)
    ctx.free(d_in)
    plan.close()


def test_index_and_density_at_max_n(pkg, ctx, cu, rig):
    """sp_plan_execute_index against the oracle's image; sp_plan_execute_density with a map of 16 colours (one of 256 makes a reply of
    1 GiB) against densityref.expected."""
    plan, d_in, nbytes = rig
    data, win, bn, _ = _max_n()
    n, lut = MAX_N, base._lut()
    want = pyoracle.render(FMT4, data, n, win, bn, GAIN, RANGE, lut, W4)
    assert plan.index_kernel_name_for(nbytes, W4) == "render_extract" and plan.kernel_name(nbytes, W4) == "scratch_radix2"
    ptrs, blk = shapes._alloc(ctx, W4, n, len(lut), 0)
    try:
        plan.execute_index(d_in, nbytes, W4, **ptrs)
        ctx.synchronize()
        got = shapes._read(ctx, ptrs, blk, W4, n, len(lut), "index at SP_MAX_N")
    finally:
        shapes._free(ctx, ptrs, blk)
    shapes.same(got, want, "index at SP_MAX_N")
    RAN.add("index")

    L = 16
    lut16 = lut[::16].copy()
    lut16[:, 0] = np.arange(L)
    want16 = pyoracle.render(FMT4, data, n, win, bn, GAIN, RANGE, lut16, W4)
    exp = densityref.expected(want16, n, L, W4, False)
    assert exp.shape == (n, L) and int(exp.sum()) == W4 * n and (exp.sum(axis=0) > 0).sum() >= 4
    plan16, out = ctx.plan(FMT4, n, win, bn, GAIN, RANGE, lut16), _Dev(ctx, 4 * n * L)
    try:
        plan16.execute_density(d_in, nbytes, W4, out.ptr)
        ctx.synchronize()
        got = out.read(np.uint32, "density at SP_MAX_N").reshape(n, L)
    finally:
        out.free()
        plan16.close()
    assert np.array_equal(got, exp.astype(np.uint32)), "density at SP_MAX_N: %d of %d counts differ" % (int((got != exp).sum()), exp.size)
    RAN.add("density")


@functools.lru_cache(maxsize=None)
def _mean_want():
    return meanref.expected(_max_n()[3])


@pytest.mark.parametrize("window", [0, 8 * MAX_N], ids=["default_window", "one_frame"])
def test_mean_at_max_n(ctx, rig, window):
    from test_mean_gpu import _execute_mean
    plan, d_in, nbytes = rig
    assert plan.mean_kernel_name_for(nbytes, W4) == "scratch_power+mean"
    ctx.set_mean_window(window)
    try:
        got = _execute_mean(ctx, plan, d_in, nbytes, W4, MAX_N, "mean at SP_MAX_N")
    finally:
        ctx.set_mean_window(0)
    meanref.assert_same(got, _mean_want(), "mean at SP_MAX_N, window %d" % window)
    RAN.add("mean_one_frame" if window else "mean")


def test_bandpower_and_track_at_max_n(ctx, rig):
    from test_band_gpu import _execute_bandpower
    from test_track_gpu import _execute_track
    plan, d_in, nbytes = rig
    bands, sums, _, _ = _band_series()
    assert plan.bandpower_kernel_name_for(nbytes, W4) == "scratch_power+bands" and plan.track_kernel_name_for(nbytes, W4) == "scratch_power+track"
    bandref.assert_same(_execute_bandpower(ctx, plan, d_in, nbytes, W4, bands, "bands at SP_MAX_N"), sums, "bands at SP_MAX_N")
    RAN.add("bandpower")
    want = trackref.expected(_max_n()[3], bands)
    trackref.assert_same(_execute_track(ctx, plan, d_in, nbytes, W4, bands, "track at SP_MAX_N"), want, "track at SP_MAX_N")
    RAN.add("track")


def test_occupancy_at_max_n(ctx, rig):
    from test_occupancy_gpu import _execute_occupancy
    plan, d_in, nbytes = rig
    plane, bands = _max_n()[3], bandref.standard_bands(MAX_N)
    thr = occref.planted_thresholds(plane)
    want = occref.expected(plane, thr, bands)
    assert {0, 1, 2, 3} <= set(np.unique(want[0]).tolist())
    assert plan.occupancy_kernel_name_for(nbytes, W4) == "scratch_power+occupancy"
    occref.assert_same(_execute_occupancy(ctx, plan, d_in, nbytes, W4, thr, bands, "occupancy at SP_MAX_N"), want, "occupancy at SP_MAX_N")
    RAN.add("occupancy")


@pytest.mark.parametrize("window", [0, 8 * MAX_N], ids=["default_window", "one_frame"])
def test_quantile_at_max_n(ctx, rig, window):
    from test_quantile_gpu import _execute_quantile
    plan, d_in, nbytes = rig
    ranks = quantileref.standard_ranks(W4)
    want = quantileref.expected(_max_n()[3], ranks)
    assert plan.quantile_kernel_name_for(nbytes, W4) == "scratch_power+quantile"
    ctx.set_mean_window(window)
    try:
        got = _execute_quantile(ctx, plan, d_in, nbytes, W4, ranks, "quantile at SP_MAX_N")
    finally:
        ctx.set_mean_window(0)
    quantileref.assert_same(got, want, "quantile at SP_MAX_N, window %d" % window)
    RAN.add("quantile_one_frame" if window else "quantile")


def test_bursts_and_pulses_at_max_n(ctx, rig):
    import test_bursts_gpu as tb
    import test_pulses_gpu as tp
    plan, d_in, nbytes = rig
    bands, sums, hi, lo = _band_series()
    m = 4
    assert plan.bursts_kernel_name_for(nbytes, W4) == "scratch_power+bursts" and plan.pulses_kernel_name_for(nbytes, W4) == "scratch_power+pulses"
    tb.assert_same(tb._execute_bursts(ctx, plan, d_in, nbytes, W4, bands, hi, lo, m, "bursts at SP_MAX_N"), burstref.expected(sums, hi, lo, m),
                   "bursts at SP_MAX_N")
    RAN.add("bursts")
    tp.assert_same(tp._execute_pulses(ctx, plan, d_in, nbytes, W4, bands, hi, lo, m, "pulses at SP_MAX_N"), pulseref.expected(sums, hi, lo, m),
                   "pulses at SP_MAX_N")
    RAN.add("pulses")


def test_resident_planes_of_any_row_count(ctx):
    """sp_power_mean, sp_power_occupancy and sp_power_quantile take a plane of any n: 2^20 - 3 rows, two frames."""
    from test_mean_gpu import _power_mean
    from test_occupancy_gpu import _power_occupancy
    from test_quantile_gpu import _power_quantile
    n, width = MAX_N - 3, 2
    rng = np.random.default_rng(20)
    plane = rng.random((width, n)) * np.exp2(rng.integers(-40, 40, (width, n)))
    what = "n = 2^20 - 3"
    meanref.assert_same(_power_mean(ctx, plane, what), meanref.expected(plane), "sp_power_mean " + what)
    i = np.arange(n)     # a value of the row itself, the next one above a value of the row, a value in between
    thr, bands = np.where(i % 3 == 0, plane[0], np.where(i % 3 == 1, np.nextafter(plane[1], np.inf), 0.5)), [(0, n), (n - 70, n), (4095, 4097)]
    occref.assert_same(_power_occupancy(ctx, plane, thr, bands, what), occref.expected(plane, thr, bands), "sp_power_occupancy " + what)
    ranks = quantileref.standard_ranks(width)
    quantileref.assert_same(_power_quantile(ctx, plane, ranks, what), quantileref.expected(plane, ranks), "sp_power_quantile " + what)
    RAN.add("any_n")


def test_twice_max_n_is_refused_and_writes_nothing(pkg, ctx):
    """n = 2^21: SP_ERR_UNSUPPORTED from sp_plan_create, sp_render and sp_render_power; no reply byte is touched."""
    n = 2 * MAX_N
    data = np.zeros(2 * (n + 8), np.uint8)
    win, lut = np.ones(n), base._lut()
    with pytest.raises(pkg.SpectroplotError) as e:
        ctx.plan("CU8", n, win, 1.0, GAIN, RANGE, lut)
    assert e.value.status == -4
    L = pkg.Library.get().L
    fid = pkg.parse_format("CU8")[0]
    req, keep = pkg.binding._make_request(fid, n, win, 1.0, GAIN, RANGE, lut, False, False)
    out, mm, rep = pkg.binding._host_reply(2, n, len(lut), fill=0xAB)
    import ctypes as C
    before = {k: v.copy() for k, v in out.items()}
    assert L.sp_render(ctx.h, C.byref(req), data.ctypes.data_as(C.c_void_p), data.size, 2, C.byref(rep)) == -4
    assert all(np.array_equal(out[k], before[k]) for k in out) and (mm == float(0xAB)).all()
    plane = np.full(2 * n, np.float64(-1.5))
    assert L.sp_render_power(ctx.h, C.byref(req), data.ctypes.data_as(C.c_void_p), data.size, 2, 0, plane.ctypes.data_as(C.c_void_p)) == -4
    assert (plane == -1.5).all()
    RAN.add("refused")


# ------------------------------------------------------------------------------------------------------------------ completeness
def test_zz_every_case_ran(cu):
    """Runs last in the module: every case has run (and passed) on this part, none skipped."""
    ids = {c["id"] for c in CASES} | set(CONSUMERS)
    assert len(ids) == len(CASES) + len(CONSUMERS)
    assert RAN == ids, "%d of %d cases ran on %d CUs; missing %s" % (len(RAN), len(ids), cu, sorted(ids - RAN))
    assert last_groups() == {1, 2, 3, 4}
