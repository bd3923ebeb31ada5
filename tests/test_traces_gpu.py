"""Per-bin min / max traces on the GPU (sp_plan_execute_traces, sp_render_traces): both arrays compared bit for bit with the fold of
the oracle's dB plane (tests/tracesref.py), through both frame loops (k_frames_traces and the portable k_scratch_traces) and both entry
points, into output buffers that hold garbage before the call.

The measurement that goes with the feature is not asserted here (tools/traces_bench.py)."""
import ctypes as C

import numpy as np
import pytest

import launchref
import siggen
import tracesref
from __graft_entry__ import load_package
from oracle import pyoracle
from test_gpu_parity import FROM_HOST, _assert_same as assert_same_reply

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 31337, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
GARBAGE = 0xAB
FRAME_SIZES = [64, 128, 256, 512, 1024]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _execute(ctx, plan, data, width, n):
    """sp_plan_execute_traces on device buffers filled with garbage; the two arrays as numpy."""
    d_in = ctx.alloc(max(data.size, 16))
    d_min, d_max = ctx.alloc(8 * n), ctx.alloc(8 * n)
    try:
        ctx.memset(d_min, GARBAGE, 8 * n)
        ctx.memset(d_max, GARBAGE, 8 * n)
        if data.size:
            ctx.upload(d_in, data)
        plan.execute_traces(d_in, data.size, width, d_min, d_max)
        ctx.synchronize()
        return {"trace_min": ctx.download(d_min, 8 * n, np.float64), "trace_max": ctx.download(d_max, 8 * n, np.float64)}
    finally:
        for p in (d_in, d_min, d_max):
            ctx.free(p)


def _garbage():
    return float(np.frombuffer(bytes([GARBAGE]) * 8, np.float64)[0])


def _check_case(ctx, fmt, n, width, data, ch=False, main=True, window="hann", gain=3.0, rng=50.0, lut=None, win=None):
    """Reference once; sp_plan_execute_traces automatically and forced onto the portable kernel; sp_render_traces.  Returns the
    expected arrays."""
    if win is None:
        win, weight = pyoracle.window(window, n)
        bn = 1.0 / weight
    else:
        bn = 1.0 / n
    want = tracesref.expected(fmt, data, n, win, bn, gain, rng, width, ch)
    if main:
        # the comparison below can only tell a wrong fold from a right one if the fold has moved every bin and the bins differ
        assert not (want["trace_min"] == 0.0).any() and not (want["trace_max"] == -200.0).any()
        assert len(np.unique(want["trace_min"])) >= n // 2 and len(np.unique(want["trace_max"])) >= n // 2
    if lut is None:
        lut = tracesref._LUT
    plan = ctx.plan(fmt, n, win, bn, gain, rng, lut, ch)
    try:
        covered = n in FRAME_SIZES and np.isfinite(win).all()
        assert plan.traces_kernel_name_for(data.size, width) == ("frames_traces" if covered else "scratch_traces")
        got_auto = _execute(ctx, plan, data, width, n)
        tracesref.assert_same(got_auto, want, "%s n=%d W=%d automatic" % (fmt, n, width))
        plan.force_kernel("scratch")
        assert plan.traces_kernel_name_for(data.size, width) == "scratch_traces"
        got_portable = _execute(ctx, plan, data, width, n)
        tracesref.assert_same(got_portable, want, "%s n=%d W=%d portable" % (fmt, n, width))
        tracesref.assert_same(got_auto, got_portable, "automatic vs portable")
        try:
            plan.force_kernel("frames")          # (refused where k_frames does not cover the plan's renders: the force stays)
        except Exception as e:
            assert getattr(e, "status", None) == -4
            plan.force_kernel("auto")
        assert plan.traces_kernel_name_for(data.size, width) == ("frames_traces" if covered else "scratch_traces")
    finally:
        plan.close()
    got = ctx.render_traces(fmt, data, n, win, bn, gain, rng, width, ch, lut=lut, fill=_garbage())
    tracesref.assert_same(got, want, "%s n=%d W=%d sp_render_traces" % (fmt, n, width))
    return want


def _capture(fmt, n, width, stride_num, stride_den=1, extra=0):
    """A capture whose stride is stride_num / stride_den samples (exactly, for width >= 2)."""
    samples = n + (max(width, 1) - 1) * stride_num // stride_den + extra
    return siggen.generate(fmt, GEN, samples)


# ---- (a) every size of the frame loop at widths of a few groups, (b) the portable kernel's own sizes -----------------------------------
@pytest.mark.parametrize("n,width", [(64, 700), (128, 333), (256, 150), (512, 77), (1024, 41)])
def test_frame_loop_sizes(ctx, n, width):
    _check_case(ctx, "CS16", n, width, _capture("CS16", n, width, n // 2 + 3))


@pytest.mark.parametrize("n,width", [(16, 64), (2048, 33), (8192, 9)])
def test_portable_kernel_sizes(ctx, n, width):
    _check_case(ctx, "CS16", n, width, _capture("CS16", n, width, n // 2 + 3))


# ---- (c) every loader ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("fmt", ["CU4", "CS8", "CS12", "CU12", "CU16", "CS32", "CF32", "CF64", "CU64"])
def test_every_loader(ctx, fmt, n):
    width = 45
    _check_case(ctx, fmt, n, width, _capture(fmt, n, width, n + 7))


# ---- (d) L/R split ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width", [("CS16", 64, 300), ("CF32", 256, 90), ("CU8", 512, 50), ("CF32", 1024, 37), ("CF64", 1024, 20),
                                         ("CS12", 2048, 12)])
def test_channel_mode(ctx, fmt, n, width):
    want = _check_case(ctx, fmt, n, width, _capture(fmt, n, width, n // 3 + 1), ch=True, main=False)
    # the split forces bin n/2 to zero (row 0): -inf below, the start value above; every other row has moved and the rows differ
    assert want["trace_min"][0] == -np.inf and want["trace_max"][0] == -200.0
    assert not (want["trace_min"][1:] == 0.0).any() and not (want["trace_max"][1:] == -200.0).any()
    assert len(np.unique(want["trace_max"])) >= n // 2


# ---- (e) strides, tiny widths, a last frame past the capture ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [128, 1024, 4096])
def test_fractional_stride_overlap_and_sparse(ctx, n):
    _check_case(ctx, "CU8", n, 37, siggen.generate("CU8", GEN, n + 36 * n + 17))          # fractional, just above n
    _check_case(ctx, "CU8", n, 50, _capture("CU8", n, 50, n // 5))                        # stride < n
    _check_case(ctx, "CS16", n, 23, _capture("CS16", n, 23, 2 * n + 5, extra=3))          # stride >= 2 n, fractional


@pytest.mark.parametrize("n", [64, 1024, 2048])
def test_width_zero_and_one(ctx, n):
    data = siggen.generate("CS16", GEN, 3 * n)
    want = _check_case(ctx, "CS16", n, 0, data, main=False)
    assert (want["trace_min"] == 0.0).all() and (want["trace_max"] == -200.0).all()
    _check_case(ctx, "CS16", n, 1, data)
    want = _check_case(ctx, "CS16", n, 0, np.zeros(0, np.uint8), main=False)              # ... and no capture at all
    assert (want["trace_max"] == -200.0).all()


@pytest.mark.parametrize("n", [256, 1024, 2048])
def test_last_frame_ends_past_the_capture(ctx, n):
    """An odd byte count of CU8: sampleCount has a half sample, the last frame starts half a sample late and reads one sample past the
    typed view (undefined -> NaN in the reference): not in bounds, the generic loaders."""
    width = 40
    data = siggen.generate("CU8", GEN, n + 39 * (n // 2))
    data = np.concatenate([data, np.array([77], np.uint8)])
    want = _check_case(ctx, "CU8", n, width, data, main=False)
    ref = pyoracle.render("CU8", data, n, pyoracle.window("hann", n)[0], 1.0, 0.0, 50.0, tracesref._LUT, width, planes=True)
    assert np.isnan(ref["abs2"][-1]).all() and np.isfinite(ref["abs2"][:-1]).all()     # the case is what its name says
    assert not (want["trace_min"] == 0.0).any()


# ---- (f) NaN and infinities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024, 2048])
def test_a_bin_that_is_nan_in_every_column_keeps_the_start_values(ctx, n):
    """Rectangular taper, stride n.  An infinite I sample at position 1 of a frame leaves two bins NaN and the others infinite; a NaN
    sample leaves every bin NaN.  Every column has one or the other: two rows stay at (0, -200), the others reach +inf above."""
    width = 24
    data = siggen.generate("CF32", GEN, n * width)
    f = data.view("<f4").reshape(-1, 2)
    for x in range(width):
        if x % 3 == 2:
            f[x * n + 5 + x, 1] = np.nan
        else:
            f[x * n + 1, 0] = np.inf if x % 2 else -np.inf
    want = _check_case(ctx, "CF32", n, width, data, main=False, win=np.ones(n))
    start = (want["trace_min"] == 0.0) & (want["trace_max"] == -200.0)
    assert start.sum() == 2 and (want["trace_max"][~start] == np.inf).all()


@pytest.mark.parametrize("n", [128, 1024, 2048])
def test_nan_in_some_columns_gives_way_to_numbers(ctx, n):
    width = 30
    data = siggen.generate("CF32", GEN, n + 29 * (n + 3))
    f = data.view("<f4").reshape(-1, 2)
    f[3 * (n + 3) + 7, 0] = np.nan
    f[7 * (n + 3) + n - 1, 1] = np.nan
    f[11 * (n + 3) + 1, 0] = np.inf
    f[12 * (n + 3) + n // 2, 1] = -np.inf
    want = _check_case(ctx, "CF32", n, width, data, main=False)
    assert not (want["trace_min"] == 0.0).any() and np.isfinite(want["trace_min"]).all()
    assert (want["trace_max"] == np.inf).any()


def test_non_finite_taper_takes_the_portable_kernel(ctx):
    n, width = 256, 20
    win = pyoracle.window("hann", n)[0].copy()
    win[17] = np.inf
    _check_case(ctx, "CS16", n, width, _capture("CS16", n, width, n), main=False, win=win)


# ---- (g) silence ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n", [("CS16", 64), ("CF32", 1024), ("CS8", 4096)])
def test_all_zero_capture(ctx, fmt, n):
    width = 19
    data = np.zeros(siggen.SAMPLE_WIDTH[fmt] * (n + 18 * (n + 1)), np.uint8)
    want = _check_case(ctx, fmt, n, width, data, main=False)
    assert (want["trace_min"] == -np.inf).all() and (want["trace_max"] == -200.0).all()


# ---- (h) the identity with sp_render -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 512, 130, False), ("CF32", 1024, 70, True), ("CU8", 2048, 20, False)])
def test_traces_fold_to_sp_renders_dbfs_range(ctx, fmt, n, width, ch):
    data = _capture(fmt, n, width, n + n // 4 + 1)
    win, weight = pyoracle.window("blackmanHarris", n)
    lut = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)
    reply = ctx.render(fmt, data, n, win, 1.0 / weight, 6.0, 40.0, lut, width, ch)
    got = ctx.render_traces(fmt, data, n, win, 1.0 / weight, 6.0, 40.0, width, ch, lut=lut, fill=_garbage())
    assert tracesref.same_bits(got["trace_min"].min(), reply["dBfs_min"]) and tracesref.same_bits(got["trace_max"].max(), reply["dBfs_max"])
    assert reply["dBfs_min"] < 0.0 and reply["dBfs_max"] > -200.0


def test_lut_length_and_edge_ranges_do_not_push_a_request_off_the_frame_loop(ctx):
    """A 1-entry colour map, one of 4096 entries and a range whose edges leave the f32 range: k_frames covers none of them."""
    n, width = 256, 60
    data = _capture("CS16", n, width, n // 2)
    for lut, rng in ((np.zeros((1, 3), np.uint8), 50.0), (np.zeros((4096, 3), np.uint8), 50.0), (tracesref._LUT, 1e-3)):
        _check_case(ctx, "CS16", n, width, data, lut=lut, rng=rng)


# ---- (i) the host entry point's upload plan ------------------------------------------------------------------------------------------------
def _device_traces(ctx, fmt, n, width, data, win, bn):
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, tracesref._LUT)
    try:
        return _execute(ctx, plan, data, width, n)
    finally:
        plan.close()


def test_packed_and_chunked_sp_render_traces(ctx):
    """stride = 1.5 n and 18 MiB of frames: the samples travel packed (only what the frames read) and in chunks, the extremes
    accumulate over the chunks."""
    fmt, n, width = "CF32", 1024, 2304
    data = _capture(fmt, n, width, 3 * n, 2)
    assert width * n * 8 >= 16 << 20 and width >= 1024      # the documented threshold of a chunked upload
    win, weight = pyoracle.window("hann", n)
    want = _device_traces(ctx, fmt, n, width, data, win, 1.0 / weight)
    assert not (want["trace_min"] == 0.0).any() and len(np.unique(want["trace_max"])) >= n // 2
    got = ctx.render_traces(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, fill=_garbage())
    tracesref.assert_same(got, want, "packed, chunked")
    assert width * n * 8 <= ctx.last_upload_bytes() < data.size * 3 // 4


def test_chunked_contiguous_sp_render_traces(ctx):
    """Overlapping frames, 20 MiB: the capture travels whole, in chunks that end with the last frame of their range."""
    fmt, n, width = "CS16", 512, 20000
    data = _capture(fmt, n, width, 262)
    assert data.size >= 16 << 20
    win, weight = pyoracle.window("hann", n)
    want = _device_traces(ctx, fmt, n, width, data, win, 1.0 / weight)
    got = ctx.render_traces(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, fill=_garbage())
    tracesref.assert_same(got, want, "contiguous, chunked")
    assert ctx.last_upload_bytes() == data.size


def test_chunked_contiguous_sp_render_traces_on_the_portable_kernel(ctx):
    """n = 2048 (scratch_traces), stride n, 16 MiB at width 1024 - the smallest request the streamer cuts - against the oracle."""
    fmt, n, width = "CF32", 2048, 1024
    data = _capture(fmt, n, width, n)
    assert data.size >= 16 << 20
    win, weight = pyoracle.window("hann", n)
    want = tracesref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, False)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, tracesref._LUT)
    try:
        assert plan.traces_kernel_name_for(data.size, width) == "scratch_traces"
    finally:
        plan.close()
    got = ctx.render_traces(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, fill=_garbage())
    tracesref.assert_same(got, want, "contiguous, chunked, portable")
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size


def test_chunked_sp_render_traces_waits_for_a_queued_execute_from_host(pkg, ctx):
    """sp_plan_execute_from_host returns with its copies and kernels still queued on the context's staging buffer; a chunked
    sp_render_traces on the same context, called WITHOUT a synchronisation in between, must not upload over them: the queued render
    against the oracle, the traces against sp_plan_execute_traces on a device copy, both bit for bit.  The capture sits in page-locked
    memory and the stream is kept busy before it, so that its copies really are still queued.  Then once more behind a
    synchronisation and without the busy work: the chunked request finds an idle stream, which it does not wait for."""
    r_fmt, r_n, r_lg, W, r_wf = FROM_HOST[3]                  # sparse, one packed chunk: it shares the staging buffer's first bytes
    r_data = siggen.generate(r_fmt, {"kind": "trinoise", "seed": 99 + r_n, "step": 7321, "gshift": 9, "amp": 0.5, "namp": 0.02}, 1 << r_lg)
    r_win, r_weight = pyoracle.window("blackmanHarris", r_n)
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    r_want = pyoracle.render(r_fmt, r_data, r_n, r_win, 1.0 / r_weight, 6.0, 30.0, lut, W, False, r_wf)
    fmt, n, width = "CS16", 512, 20000                        # test_chunked_contiguous_sp_render_traces' shape
    data = _capture(fmt, n, width, 262)
    assert data.size >= 16 << 20 and width >= 1024
    win, weight = pyoracle.window("hann", n)
    want = _device_traces(ctx, fmt, n, width, data, win, 1.0 / weight)
    assert not (want["trace_min"] == 0.0).any() and len(np.unique(want["trace_max"])) >= n // 2
    plan = ctx.plan(r_fmt, r_n, r_win, 1.0 / r_weight, 6.0, 30.0, lut, False, r_wf)
    sizes = [4 * W * r_n, W, W, W, 8 * 256, 8000, 16]
    ptrs = [ctx.alloc(max(s_, 16)) for s_ in sizes]
    L = ctx.lib.L
    L.sp_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.sp_host_free.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert L.sp_host_alloc(r_data.size, C.byref(h)) == 0
    pinned = np.ctypeslib.as_array(C.cast(h, C.POINTER(C.c_uint8)), shape=(r_data.size,))
    pinned[:] = r_data
    busy = ctx.alloc(1 << 30)
    try:
        # once before, so that nothing between the two calls below synchronises by itself (the traces' plan, staging buffers, streams)
        tracesref.assert_same(ctx.render_traces(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, fill=_garbage()), want, "before")
        for queued in (True, False):
            for p_, s_ in zip(ptrs, sizes):
                ctx.memset(p_, 0xA5, max(s_, 16))
            if queued:
                for _ in range(16):                            # a few ms of work ahead of the request on the context's stream
                    ctx.memset(busy, 0, 1 << 30)
            plan.execute_from_host(pinned, W, *ptrs)
            if not queued:
                ctx.synchronize()
            got = ctx.render_traces(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, fill=_garbage())
            ctx.synchronize()
            assert ctx.last_upload_bytes() == data.size
            r_got = {"rgba": ctx.download(ptrs[0], sizes[0]), "gauge_mins": ctx.download(ptrs[1], W), "gauge_maxs": ctx.download(ptrs[2], W),
                     "gauge_amps": ctx.download(ptrs[3], W), "c_hist": ctx.download(ptrs[4], 8 * 256, np.uint64),
                     "cB_hist": ctx.download(ptrs[5], 8000, np.uint64)}
            mm = ctx.download(ptrs[6], 16, np.float64)
            r_got["dBfs_min"], r_got["dBfs_max"] = float(mm[0]), float(mm[1])
            assert_same_reply(r_got, r_want)
            tracesref.assert_same(got, want, "behind a queued execute_from_host" if queued else "on an idle stream")
    finally:
        L.sp_host_free(h)
        for p_ in ptrs + [busy]:
            ctx.free(p_)
        plan.close()


def test_small_sparse_request_uploads_its_frames_only(ctx):
    fmt, n, width = "CU8", 256, 64
    data = _capture(fmt, n, width, 40 * n + 11)
    _check_case(ctx, fmt, n, width, data)
    assert ctx.last_upload_bytes() < data.size // 8


# ---- (j) refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    d_in, d_out = ctx.alloc(data.size), ctx.alloc(16 * n + 16)
    vp = C.c_void_p
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, tracesref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, tracesref._LUT)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_traces(d_in, data.size, width, d_out, d_out + 8 * n)
        assert e.value.status == -4 and "peak" in str(e.value)
        assert L.sp_plan_execute_traces(None, vp(d_in), data.size, width, vp(d_out), vp(d_out + 8 * n)) == -1
        assert L.sp_plan_execute_traces(plan.h, vp(d_in), data.size, -1, vp(d_out), vp(d_out + 8 * n)) == -1
        assert L.sp_plan_execute_traces(plan.h, None, data.size, width, vp(d_out), vp(d_out + 8 * n)) == -1
        assert L.sp_plan_execute_traces(plan.h, vp(d_in), data.size, width, vp(d_out + 4), vp(d_out + 8 * n)) == -1      # misaligned
        assert L.sp_plan_execute_traces(plan.h, vp(d_in), data.size, width, vp(d_out), vp(d_out + 8 * n + 1)) == -1
        assert L.sp_plan_traces_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
        plan.execute_traces(d_in, data.size, width, 0, d_out)              # either output may be left out
        plan.execute_traces(d_in, data.size, width, d_out, 0)
        ctx.synchronize()
    finally:
        peak.close()
        plan.close()
        ctx.free(d_in)
        ctx.free(d_out)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, tracesref._LUT, False, False, "peak")
    out = np.zeros(2 * n)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    assert L.sp_render_traces(ctx.h, C.byref(req), p(data), data.size, width, p(out), p(out[n:])) == -4
    req.detector = 0
    assert L.sp_render_traces(None, C.byref(req), p(data), data.size, width, p(out), p(out[n:])) == -1
    assert L.sp_render_traces(ctx.h, None, p(data), data.size, width, p(out), p(out[n:])) == -1
    assert L.sp_render_traces(ctx.h, C.byref(req), None, data.size, width, p(out), p(out[n:])) == -1
    assert L.sp_render_traces(ctx.h, C.byref(req), p(data), data.size, -2, p(out), p(out[n:])) == -1
    req16, keep16 = pkg.binding._make_request(pkg.parse_format("CS16")[0], n, win, 1.0 / weight, 3.0, 50.0, tracesref._LUT, False, False)
    assert L.sp_render_traces(ctx.h, C.byref(req16), p(data), 4 * 100 + 1, width, p(out), p(out[n:])) == -3


# ---- (k) launch shapes ---------------------------------------------------------------------------------------------------------------------
SHAPE_FORMATS = ["CS16", "CU8", "CF32", "CS12", "CU4"]


@pytest.mark.parametrize("regime", ["mixed", "many"])
@pytest.mark.parametrize("n", FRAME_SIZES)
def test_launch_shapes(pkg, ctx, n, regime):
    """Where the per-workgroup arrays and their single flush can go wrong: some workgroups with two groups and some with one (smallest
    gf), three groups or more for every workgroup (largest gf: rounds > 1, HALVES at n = 1024), a ragged last group, a group count
    that is no multiple of 8."""
    k = FRAME_SIZES.index(n)
    fmt, ch = SHAPE_FORMATS[(k + (regime == "many")) % 5], (k + (regime == "mixed")) % 2 == 1
    win, weight = pyoracle.window("hann", n)
    probe = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, tracesref._LUT, ch)
    cu = probe.debug_launch(16 * n, 4)["cu_count"]
    probe.close()
    gfs = launchref.reachable_gf(n)
    gf = gfs[0] if regime == "mixed" else gfs[-1]
    width = launchref.choose_width(n, cu, gf, regime, w4=False)
    assert width is not None
    gf_l, groups, grid, _ = pkg.binding.debug_frames_launch(n, 2, width, cu)          # the rule k_frames_traces launches by
    assert gf_l == gf and groups % 8 != 0 and width % gf != 0 and launchref.regime_of(groups, grid) == regime
    assert launchref.halves(n, gf) == (n == 1024 and regime == "many")
    assert width * n * 16 < 1 << 30
    data = siggen.generate(fmt, GEN, n + (width - 1) * 67 + 29)                            # a fractional stride of about 67 samples
    want = _check_case(ctx, fmt, n, width, data, ch=ch, main=not ch)
    if ch:
        assert not (want["trace_min"][1:] == 0.0).any() and len(np.unique(want["trace_max"])) >= n // 2
