"""The averaged spectrogram on the GPU (sp_power_blockmean, sp_plan_execute_blockmean, sp_render_blockmean) and the colouring of a
plane (sp_plan_power_to_index): every comparison is bit for bit - against tests/blockmeanref.py (math.fsum per column and row, divided
by the column's frames) on a synthetic plane with the hard cases planted, on the oracle's plane, and against what the library already
replies at both ends (the power plane, the mean, the index image).  Every device result lies between guard bytes and holds garbage
before the call.

The measurement that goes with the feature is not asserted here (tools/blockmean_bench.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bandref
import blockmeanref
import edgeref
import powerref
from __graft_entry__ import load_package
from oracle import pyoracle
from test_density_gpu import _hip_runtime
from test_mean_gpu import GARBAGE, GUARD, _capture, _Out, _reference, _upload

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 3, 5, 64, 130, 131, 132, 1000)
N, WIDTH = blockmeanref.N, blockmeanref.WIDTH


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.set_blockmean_direct_max(0)
    c.set_cu_count(0)
    c.close()


@functools.lru_cache(maxsize=None)
def _planted():
    plane = blockmeanref.planted_plane()
    blockmeanref.telling(plane)
    plane.setflags(write=False)
    want = {g: blockmeanref.expected(plane, g) for g in GROUPS}
    return plane, want


@pytest.fixture(scope="module")
def resident(ctx):
    """The planted plane on the device, once for the tests that read it."""
    plane, want = _planted()
    d = _upload(ctx, plane)
    yield d, plane, want
    ctx.free(d)


def _power_blockmean(ctx, d_plane, n, width, group, what):
    cols = blockmeanref.columns(width, group)
    out = _Out(ctx, cols * n)
    try:
        ctx.power_blockmean(d_plane, n, width, group, out.ptr)
        ctx.synchronize()
        return out.read(what).reshape(cols, n)
    finally:
        out.free()


def _execute_blockmean(ctx, plan, d_in, nbytes, width, group, n, what):
    cols = blockmeanref.columns(width, group)
    out = _Out(ctx, cols * n)
    try:
        plan.execute_blockmean(d_in, nbytes, width, group, out.ptr)
        ctx.synchronize()
        return out.read(what).reshape(cols, n)
    finally:
        out.free()


# ---- (a) the resident plane -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_resident_plane_against_fsum(ctx, resident, group):
    d, plane, want = resident
    got = _power_blockmean(ctx, d, N, WIDTH, group, "group %d" % group)
    blockmeanref.assert_same(got, want[group], "sp_power_blockmean group %d" % group)


def test_both_ends_are_what_the_library_already_replies(ctx, resident):
    d, plane, want = resident
    got = _power_blockmean(ctx, d, N, WIDTH, 1, "group 1")
    assert np.array_equal(blockmeanref.bits(got), blockmeanref.bits(plane))            # the plane's bits, its NaN the one NaN
    mean = _Out(ctx, N)
    try:
        ctx.power_mean(d, N, WIDTH, mean.ptr)
        ctx.synchronize()
        m = mean.read("mean")
    finally:
        mean.free()
    for group in (131, 132, 1000):
        got = _power_blockmean(ctx, d, N, WIDTH, group, "group %d" % group)
        assert got.shape == (1, N) and np.array_equal(blockmeanref.bits(got[0]), blockmeanref.bits(m)), group


def test_the_path_split_does_not_change_a_bit(ctx, resident):
    """Everything carried, the built default, everything direct."""
    d, plane, want = resident
    try:
        for direct_max in (1, 0, 2 ** 30):
            ctx.set_blockmean_direct_max(direct_max)
            for group in GROUPS:
                got = _power_blockmean(ctx, d, N, WIDTH, group, "direct_max %d group %d" % (direct_max, group))
                blockmeanref.assert_same(got, want[group], "direct_max %d, group %d" % (direct_max, group))
    finally:
        ctx.set_blockmean_direct_max(0)


@pytest.mark.parametrize("cu", [8, 304])
def test_the_cu_count_does_not_change_a_bit(pkg, ctx, resident, cu):
    """sp_context_debug_set_cu_count admits 1 ... the part's own count.  304 is above an MI355X's 256: where the override refuses it, the
    launch rules themselves (sp_debug_blockmean_launch, sp_debug_mean_launch - the functions the launches call) must give this plane's
    runs at 304 CUs the very grids they get at the part's own count, and those launches are the ones compared."""
    d, plane, want = resident
    b = pkg.binding
    try:
        try:
            ctx.set_cu_count(cu)
            shaped = cu
        except pkg.SpectroplotError:
            ctx.set_cu_count(0)
            shaped = _own_cu_count(ctx)
            assert shaped < cu
            for frames in range(1, WIDTH + 1):
                assert b.debug_mean_launch(N, frames, cu) == b.debug_mean_launch(N, frames, shaped), frames
                for group in GROUPS:
                    assert b.debug_blockmean_launch(N, frames, group, cu) == b.debug_blockmean_launch(N, frames, group, shaped), (frames, group)
        if shaped == 8:   # the count shapes what is launched: fewer pieces than columns, several columns per workgroup
            assert b.debug_blockmean_launch(N, WIDTH, 1, 8) == (2, 27, 5) and b.debug_blockmean_launch(N, WIDTH, 1, 256) == (2, 131, 1)
        for direct_max in (1, 2 ** 30):
            ctx.set_blockmean_direct_max(direct_max)
            for group in GROUPS:
                got = _power_blockmean(ctx, d, N, WIDTH, group, "cu %d group %d" % (cu, group))
                blockmeanref.assert_same(got, want[group], "cu %d, direct_max %d, group %d" % (cu, direct_max, group))
    finally:
        ctx.set_cu_count(0)
        ctx.set_blockmean_direct_max(0)


def _own_cu_count(ctx):
    """The part's own CU count, as sp_plan_debug_launch reports it on a context without an override."""
    win, weight = pyoracle.window("hann", 64)
    plan = ctx.plan("CU8", 64, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        return plan.debug_launch(2 * 64 * 4, 4)["cu_count"]
    finally:
        plan.close()


# ---- (b) a capture through the window ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["frames", "scratch"])
def test_capture_through_the_window(ctx, forced):
    fmt, n, width = "CU8", 256, 203
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n // 2 + 3)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d_in = _upload(ctx, data)
    try:
        if forced:
            plan.force_kernel("scratch")
        assert plan.blockmean_kernel_name_for(data.size, width) == ("scratch_power" if forced else "frames_power") + "+blockmean"
        for group in (3, 7):
            want = blockmeanref.expected(plane, group)
            got = []
            for window in (8 * n, 5 * 8 * n, 0):
                ctx.set_mean_window(window)
                got.append(_execute_blockmean(ctx, plan, d_in, data.size, width, group, n, "window %d group %d" % (window, group)))
            for g in got:
                blockmeanref.assert_same(g, want, "group %d through the window" % group)
    finally:
        ctx.set_mean_window(0)
        ctx.free(d_in)
        plan.close()


# ---- (c) host-fed and chunked -----------------------------------------------------------------------------------------------------------------
def test_host_fed_columns_straddle_chunks_and_window_blocks(ctx):
    fmt, n, width, group = "CF32", 1024, 2048, 48      # test_plane_window_gpu.py's request: the smallest the streamer cuts, on multiples of 32
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n)
    assert data.size >= 16 << 20
    want = blockmeanref.expected(plane, group)
    render = lambda db=False: ctx.render_blockmean(fmt, data, n, win, bn, 3.0, 50.0, width, group, db=db, fill=GARBAGE)
    try:
        ctx.set_mean_window(5 * 8 * n)
        got = render()
        assert ctx.last_chunks() > 1
    finally:
        ctx.set_mean_window(0)
    blockmeanref.assert_same(got, want, "a window of 5 frames")
    default = render()
    assert ctx.last_chunks() > 1
    assert np.array_equal(blockmeanref.bits(got), blockmeanref.bits(default)), "the window changed the reply"
    # the dB form is the dB of the means
    db = render(db=True)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    d = _upload(ctx, default)
    try:
        plan.power_to_db(d, default.size, d)
        ctx.synchronize()
        assert np.array_equal(blockmeanref.bits(db), ctx.download(d, 8 * default.size, np.uint64).reshape(db.shape))
    finally:
        ctx.free(d)
        plan.close()


# ---- (d) refusals and the empty request -------------------------------------------------------------------------------------------------------
def test_refusals_and_width_zero(pkg, ctx, resident):
    d, plane, want = resident
    fmt, n, width = "CU8", 256, 203
    data, win, bn, _, _ = _reference(fmt, n, width, False, n // 2 + 3)
    out = _Out(ctx, 2 * WIDTH * N)
    d_in = _upload(ctx, data)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    peak = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, detector="peak")
    try:
        def status(call):
            with pytest.raises(pkg.SpectroplotError) as ei:
                call()
            return ei.value.status

        assert status(lambda: ctx.power_blockmean(d, N, WIDTH, 0, out.ptr)) == -1
        assert status(lambda: ctx.power_blockmean(d, N, WIDTH, 5, out.ptr + 4)) == -1
        assert status(lambda: ctx.power_blockmean(d, N, WIDTH, 5, 0)) == -1
        assert status(lambda: plan.execute_blockmean(d_in, data.size, width, 0, out.ptr)) == -1
        assert status(lambda: plan.execute_blockmean(d_in, data.size, width, 7, out.ptr + 4)) == -1
        assert status(lambda: peak.execute_blockmean(d_in, data.size, width, 7, out.ptr)) == -4
        assert status(lambda: peak.execute_blockmean(d_in, data.size, width, 0, out.ptr)) == -1          # the group's refusal comes first
        assert status(lambda: ctx.render_blockmean(fmt, data, n, win, bn, 3.0, 50.0, width, 0)) == -1
        ctx.synchronize()
        # width 0 writes nothing, with or without an output
        ctx.power_blockmean(0, N, 0, 5, 0)
        ctx.power_blockmean(0, N, 0, 5, out.ptr)
        plan.execute_blockmean(d_in, data.size, 0, 7, out.ptr)
        assert ctx.render_blockmean(fmt, data, n, win, bn, 3.0, 50.0, 0, 7).shape == (0, n)
        ctx.synchronize()
        assert (out.read("refused or empty").view(np.uint8) == GARBAGE).all()
        # peak plans only colour
        d_ix, d_p = ctx.alloc(n * width), ctx.alloc(8 * n * width)
        try:
            ctx.memset(d_p, 0, 8 * n * width)
            peak.power_to_index(d_p, width, d_ix)
            assert status(lambda: plan.power_to_index(d_p + 4, width, d_ix)) == -1
            assert status(lambda: plan.power_to_index(d_p, width, 0)) == -1
            plan.power_to_index(0, 0, 0)
            ctx.synchronize()
            assert (ctx.download(d_ix, n * width) == 0).all()
        finally:
            ctx.free(d_ix)
            ctx.free(d_p)
    finally:
        out.free()
        ctx.free(d_in)
        plan.close()
        peak.close()


# ---- (e) the reply is a plane the other consumers read ------------------------------------------------------------------------------------------
def test_band_sums_of_the_block_mean_plane(ctx, resident):
    d, plane, want = resident
    group = 5
    cols = blockmeanref.columns(WIDTH, group)
    bands = [(0, N), (6, 14), (64, 96), (95, 96), (40, 40)]
    means, series = _Out(ctx, cols * N), _Out(ctx, len(bands) * cols)
    try:
        ctx.power_blockmean(d, N, WIDTH, group, means.ptr)
        ctx.power_bands(means.ptr, N, cols, bands, series.ptr)
        ctx.synchronize()
        bandref.assert_same(series.read("bands").reshape(len(bands), cols), bandref.expected(want[group], bands), "bands of the block means")
    finally:
        means.free()
        series.free()


# ---- (f) replay from a captured graph ---------------------------------------------------------------------------------------------------------
def test_block_means_and_colouring_replay_from_a_graph(pkg):
    hip = _hip_runtime(pkg)
    fmt, n, width, group = "CU8", 256, 203, 7
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want = blockmeanref.expected(plane, group)
    cols = want.shape[0]
    lut = edgeref.lut(256)
    own = pkg.Context(0)
    stream, graph, exe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        plan = own.plan(fmt, n, win, bn, 3.0, 50.0, lut)
        d_in = _upload(own, data)
        means = _Out(own, cols * n)
        ix_bytes = (cols * n + 7) // 8
        image = _Out(own, ix_bytes)
        assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
        own.set_stream(stream.value)
        own.set_mean_window(5 * 8 * n)             # columns straddle the window's blocks: both paths are recorded

        def queue():
            plan.execute_blockmean(d_in, data.size, width, group, means.ptr)
            plan.power_to_index(means.ptr, cols, image.ptr)

        queue()                                    # (outside a capture: the workspaces exist from here on)
        own.synchronize()
        first = image.read("outside the capture").view(np.uint8)[:cols * n].copy()
        for o, size in ((means, 8 * cols * n), (image, 8 * ix_bytes)):
            own.memset(o.base, GARBAGE, size + 2 * GUARD)
        own.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0               # hipStreamCaptureModeThreadLocal
        try:
            queue()
        finally:
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
        assert graph.value
        assert (means.read("recorded, not run").view(np.uint8) == GARBAGE).all()
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
        assert hip.hipGraphLaunch(exe, stream) == 0
        own.synchronize()
        blockmeanref.assert_same(means.read("replayed").reshape(cols, n), want, "replayed block means")
        replayed = image.read("replayed").view(np.uint8)[:cols * n]
        assert np.array_equal(replayed, first) and np.array_equal(replayed, _colour(want, 3.0, 50.0, 256, bn, False))
        plan.close()
        means.free()
        image.free()
        own.free(d_in)
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        own.set_mean_window(0)
        own.set_stream(None)
        own.close()
        if stream.value:
            hip.hipStreamDestroy(stream)


# ---- (g) sp_plan_power_to_index ---------------------------------------------------------------------------------------------------------------
def _gray(plane, gain, rng, lut_len, block_norm):
    """The colour index of every value of a plane, u8 of its shape, from the reference's arithmetic alone: the number of the oracle's own
    colour steps (edgeref.index_edges: bisection over edgeref.Scales.gray, the oracle's log10) at or below the value; NaN is 0."""
    edges, _ = edgeref.index_edges(gain, rng, lut_len, block_norm)
    assert len(edges) == lut_len - 1
    with np.errstate(all="ignore"):
        return np.where(np.isnan(plane), 0, np.searchsorted(edges, plane, side="right")).astype(np.uint8)


def _colour(plane, gain, rng, lut_len, block_norm, waterfall):
    """... laid out as "Indexed image replies" lays an index image: j = x + width * y, or j = n * (width - 1 - x) + (n - 1 - y)."""
    g = _gray(plane, gain, rng, lut_len, block_norm)
    return g[::-1, ::-1].reshape(-1).copy() if waterfall else g.T.reshape(-1).copy()


def _index_of(ctx, plan, d_plane, n, width, what):
    size = (n * width + 7) // 8
    out = _Out(ctx, size)
    try:
        plan.power_to_index(d_plane, width, out.ptr)
        ctx.synchronize()
        return out.read(what).view(np.uint8)[:n * width].copy()
    finally:
        out.free()


@pytest.mark.parametrize("lut_len", [2, 256])
@pytest.mark.parametrize("waterfall", [False, True], ids=["spectrogram", "waterfall"])
@pytest.mark.parametrize("width", [1, 37, 300])
@pytest.mark.parametrize("n", [64, 1024])
def test_colouring_a_plane(ctx, n, width, waterfall, lut_len):
    fmt, gain, rng, group = "CS16", 3.0, 50.0, 7
    data = _capture(fmt, n, width, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    bn = 1.0 / weight
    plan = ctx.plan(fmt, n, win, bn, gain, rng, edgeref.lut(lut_len), False, waterfall)
    d_in = _upload(ctx, data)
    d_plane, d_ix = ctx.alloc(8 * width * n), ctx.alloc(width * n + 16)
    cols = blockmeanref.columns(width, group)
    means = _Out(ctx, cols * n)
    what = "n=%d W=%d %s lut %d" % (n, width, "waterfall" if waterfall else "spectrogram", lut_len)
    try:
        # the plan's own plane: sp_plan_execute_index's image, byte for byte
        plan.execute_power(d_in, data.size, width, d_plane)
        plan.execute_index(d_in, data.size, width, index=d_ix)
        ctx.synchronize()
        image = ctx.download(d_ix, width * n)
        assert np.array_equal(_index_of(ctx, plan, d_plane, n, width, what), image), what
        if width > 1:
            assert len(np.unique(image)) > 1, what + ": the image is one colour"
        # a block-mean plane: the reference's arithmetic on blockmeanref's plane
        plane = ctx.download(d_plane, 8 * width * n, np.float64).reshape(width, n)
        want = blockmeanref.expected(plane, group)
        plan.execute_blockmean(d_in, data.size, width, group, means.ptr)
        ctx.synchronize()
        blockmeanref.assert_same(means.read(what).reshape(cols, n), want, what)
        assert np.array_equal(_index_of(ctx, plan, means.ptr, n, cols, what), _colour(want, gain, rng, lut_len, bn, waterfall)), what
        # a plane with the values that decide planted: 0, +inf, NaN, and two ulps either side of three edges
        edges, _ = edgeref.index_edges(gain, rng, lut_len, bn)
        pick = edges[[0, len(edges) // 2, -1]]
        near = (pick.view(np.int64)[:, None] + np.arange(-2, 3, dtype=np.int64)[None, :]).view(np.float64).reshape(-1)
        planted = np.array(plane)
        spots = np.random.default_rng(n + width).choice(planted.size, len(near) + 3, replace=False)
        planted.reshape(-1)[spots] = np.concatenate([near, [0.0, np.inf, np.nan]])
        ctx.upload(d_plane, planted.view(np.uint8).reshape(-1))
        want_ix = _colour(planted, gain, rng, lut_len, bn, waterfall)
        got_ix = _index_of(ctx, plan, d_plane, n, width, what)
        assert np.array_equal(got_ix, want_ix), what
        flat = _gray(planted, gain, rng, lut_len, bn).reshape(-1)
        scales = edgeref.Scales(gain, rng, lut_len, bn)
        assert list(flat[spots[:len(near)]]) == [scales.gray(float(v)) for v in near]                # the steps are the reference's own
        assert list(flat[spots[-3:]]) == [0, lut_len - 1, 0] and len(set(flat[spots[:len(near)]])) >= min(lut_len, 4)
    finally:
        means.free()
        for p in (d_in, d_plane, d_ix):
            ctx.free(p)
        plan.close()
