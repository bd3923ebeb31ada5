"""Indexed image replies on the device at the smallest shapes: sp_plan_execute_index, sp_render_index, sp_index_to_rgba.

Every comparison is bit for bit with the oracle (tests/indexref.py: the LUT is injective with R = index, so the expected index image is
the oracle's rgba[..., 0]); output buffers start as garbage, the index image lies between guard bytes, and gauges, both histograms and
the dBfs bit patterns are compared along with the image."""
import numpy as np
import pytest

import indexref
import peakref
import siggen
import test_index_launch_shapes_gpu as shapes
import test_launch_shapes_gpu as base
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GAIN, RANGE = base.GAIN, base.RANGE
pkg, ctx = base.pkg, base.ctx
GEN = {"kind": "trinoise", "seed": 977, "step": 4099, "gshift": 9, "amp": 0.45, "namp": 0.03}


def _request(fmt, n, W, samples, seed=0):
    data = siggen.generate(fmt, dict(GEN, seed=GEN["seed"] + seed), samples)
    win, weight = pyoracle.window("hann", n)
    return data, win, weight


def _execute(ctx, fmt, n, W, data, win, weight, lut, ch=False, wf=False, off=0, detector="sample", force=None, kernel=None):
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut, ch, wf, detector)
    try:
        if force:
            plan.force_kernel(force)
        if kernel:
            assert plan.index_kernel_name_for(data.size, W) == kernel
        return shapes.run(ctx, plan, data, W, n, len(lut), off, lambda d: None, "n%d W%d" % (n, W))
    finally:
        plan.close()


@pytest.mark.parametrize("wf", [False, True])
@pytest.mark.parametrize("W", [0, 1, 2, 3, 15, 16, 17, 33])
def test_smallest_widths_both_layouts(ctx, W, wf):
    n, fmt = 64, "CS16"
    data, win, weight = _request(fmt, n, W, n + 40 * max(W, 1) + 3, W)
    lut = base._lut()
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf)
    for off in (0, 1):
        got = _execute(ctx, fmt, n, W, data, win, weight, lut, wf=wf, off=off, kernel="frames_index")
        shapes.same(got, want, "W=%d wf=%d off=%d" % (W, wf, off))
    got = _execute(ctx, fmt, n, W, data, win, weight, lut, wf=wf, force="scratch", kernel="render_extract")
    shapes.same(got, want, "W=%d wf=%d render_extract" % (W, wf))


def test_capture_shorter_than_n_indexes_zero_and_odd_byte_tail(ctx):
    n, fmt, lut = 64, "CU8", base._lut()
    win, weight = pyoracle.window("hann", n)
    short = siggen.generate(fmt, GEN, 40)                          # every frame reads past the end: NaN frames, index 0
    want = pyoracle.render(fmt, short, n, win, 1.0 / weight, GAIN, RANGE, lut, 5, False, False)
    got = _execute(ctx, fmt, n, 5, short, win, weight, lut)
    shapes.same(got, want, "short capture")
    assert (got["index"] == 0).all()
    odd = np.concatenate([siggen.generate(fmt, GEN, 64 + 16 * 37), np.array([0x5A], np.uint8)])   # half a sample behind the last one
    want = pyoracle.render(fmt, odd, n, win, 1.0 / weight, GAIN, RANGE, lut, 38, False, True)
    got = _execute(ctx, fmt, n, 38, odd, win, weight, lut, wf=True)
    shapes.same(got, want, "odd byte tail")


@pytest.mark.parametrize("L", [2, 256])
def test_lut_lengths(ctx, L):
    n, fmt, W = 128, "CF32", 40
    data, win, weight = _request(fmt, n, W, n + 39 * 50)
    lut = base._lut()[:L].copy()
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, False)
    shapes.same(_execute(ctx, fmt, n, W, data, win, weight, lut, kernel="frames_index"), want, "lut_len %d" % L)


def test_refusals(pkg, ctx):
    n, fmt, W = 64, "CU8", 8
    data, win, weight = _request(fmt, n, W, 64 * 8)
    i = np.arange(300)
    long_lut = np.stack([i & 255, i >> 8, i & 255], axis=1).astype(np.uint8)
    d_in, d_ix = ctx.alloc(data.size + 16), ctx.alloc(W * n)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, long_lut)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            plan.execute_index(d_in, data.size, W, index=d_ix)
        assert e.value.status == -4                                   # SP_ERR_UNSUPPORTED: a byte cannot hold the index
        with pytest.raises(pkg.SpectroplotError) as e:
            ctx.render_index(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, long_lut, W)
        assert e.value.status == -4
    finally:
        plan.close()
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, base._lut())
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            plan.execute_index(d_in, data.size, W, index=d_ix, rgba=d_ix)
        assert e.value.status == -1                                   # SP_ERR_INVALID_ARG: rgba must be NULL
    finally:
        plan.close()
        ctx.free(d_in)
        ctx.free(d_ix)


@pytest.mark.parametrize("force", [None, "scratch"])
def test_null_index_gives_the_side_outputs_only(ctx, force):
    n, fmt, W, lut = 256, "CS8", 50, base._lut()
    data, win, weight = _request(fmt, n, W, n + 49 * 100)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, False)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut)
    ptrs, blk = shapes._alloc(ctx, W, n, len(lut), 0)
    d_in = ctx.alloc(data.size + 16)
    try:
        if force:
            plan.force_kernel(force)
        ctx.upload(d_in, data)
        plan.execute_index(d_in, data.size, W, **dict(ptrs, index=0))
        ctx.synchronize()
        got = shapes._read(ctx, ptrs, blk, W, n, len(lut), "null index")
        assert (got["index"] == 0xAB).all()
        base._same(dict(got, rgba=want["rgba"]), want, "null index")
    finally:
        shapes._free(ctx, ptrs, blk)
        ctx.free(d_in)
        plan.close()


@pytest.mark.parametrize("n,W", [(32, 21), (16384, 5)])
def test_sizes_outside_the_frame_loop_take_render_extract(ctx, n, W):
    fmt, lut = "CS16", base._lut()
    data, win, weight = _request(fmt, n, W, n + (W - 1) * (n // 2) + 1)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, n == 32)
    shapes.same(_execute(ctx, fmt, n, W, data, win, weight, lut, wf=n == 32, kernel="render_extract"), want, "n=%d" % n)


@pytest.mark.parametrize("M", [2, 3])
def test_peak_plan_takes_render_extract(ctx, M):
    n, fmt, W, lut = 128, "CU8", 37, base._lut()
    samples = n + (W - 1) * M * n + (W - 1) // 2 + 1
    data, win, weight = _request(fmt, n, W, samples)
    want = peakref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, False)
    assert want["M"] == M
    got = _execute(ctx, fmt, n, W, data, win, weight, lut, detector="peak", kernel="render_extract")
    shapes.same(got, want, "peak M=%d" % M)


@pytest.mark.parametrize("pixels,ioff,roff", [(1, 0, 0), (15, 3, 0), (16 * 300 + 7, 0, 0), (4099, 1, 4), (5000, 5, 1), (64 * 33, 0, 8)])
def test_index_to_rgba_is_the_lut_step(pkg, ctx, pixels, ioff, roff):
    """The LUT step alone on an index image that holds every value: odd pixel counts, misaligned pointers, guards around the RGBA,
    indices the map does not have.  (The comparison with a render through that map follows below.)"""
    lut = base._lut()[:200]                                           # indices 200 .. 255 are not in the map: (0, 0, 0, 255)
    index = ((np.arange(pixels) * 37 + 11) & 255).astype(np.uint8)
    d_ix, d_out = ctx.alloc(pixels + 32), ctx.alloc(4 * pixels + 2 * base.GUARD + 32)
    try:
        ctx.memset(d_out, 0xAB, 4 * pixels + 2 * base.GUARD + 32)
        ctx.upload(d_ix + ioff, index)
        ctx.index_to_rgba(d_ix + ioff, pixels, lut, d_out + base.GUARD + roff)
        ctx.synchronize()
        whole = ctx.download(d_out, 4 * pixels + 2 * base.GUARD + 32)
    finally:
        ctx.free(d_ix)
        ctx.free(d_out)
    table = np.zeros((256, 4), np.uint8)
    table[:, 3] = 255
    table[:len(lut), :3] = lut
    a = base.GUARD + roff
    assert (whole[:a] == 0xAB).all() and (whole[a + 4 * pixels:] == 0xAB).all()
    assert np.array_equal(whole[a:a + 4 * pixels].reshape(-1, 4), table[index])


def test_index_to_rgba_with_viridis_is_sp_plan_executes_rgba_with_viridis(ctx):
    """sp_index_to_rgba(index, viridis) == the RGBA sp_plan_execute writes for the same request with viridis; odd pixel count, the index
    image 1 byte and the RGBA image 4 bytes off 16-byte alignment."""
    import goldenlib
    n, fmt, W = 256, "CU8", 37
    data, win, weight = _request(fmt, n, W, n + 36 * 300)
    viridis = np.asarray(goldenlib.Golden().lut("viridis"), np.uint8).reshape(-1, 3)
    assert len(viridis) == 256 and len({tuple(r) for r in viridis.tolist()}) > 200
    got = _execute(ctx, fmt, n, W, data, win, weight, base._lut(), kernel="frames_index")
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, viridis)
    ptrs, blk = base._alloc_reply(ctx, W, n, 256, False)
    d_in, d_ix, d_out = ctx.alloc(data.size + 16), ctx.alloc(W * n + 16), ctx.alloc(4 * W * n + 32)
    try:
        ctx.upload(d_in, data)
        plan.execute(d_in, data.size, W, **ptrs)
        ctx.upload(d_ix + 1, got["index"])
        ctx.index_to_rgba(d_ix + 1, W * n, viridis, d_out + 4)
        ctx.synchronize()
        rendered = base._read_reply(ctx, ptrs, blk, W, n, 256, "viridis")["rgba"]
        assert np.array_equal(ctx.download(d_out + 4, 4 * W * n), rendered)
    finally:
        base._free_reply(ctx, ptrs, blk)
        for p in (d_in, d_ix, d_out):
            ctx.free(p)
        plan.close()


def test_execute_and_execute_index_interleave_without_a_sync(ctx):
    """sp_plan_execute, sp_plan_execute_index, sp_plan_execute queued back to back on one context: the shared request number."""
    n, fmt, W, lut = 512, "CS16", 200, base._lut()
    data, win, weight = _request(fmt, n, W, n + 199 * 300)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, False)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut)
    d_in = ctx.alloc(data.size + 16)
    r0, b0 = base._alloc_reply(ctx, W, n, len(lut), False)
    r1, b1 = shapes._alloc(ctx, W, n, len(lut), 0)
    r2, b2 = base._alloc_reply(ctx, W, n, len(lut), False)
    try:
        ctx.upload(d_in, data)
        plan.execute(d_in, data.size, W, **r0)
        plan.execute_index(d_in, data.size, W, **r1)
        plan.execute(d_in, data.size, W, **r2)
        ctx.synchronize()
        base._same(base._read_reply(ctx, r0, b0, W, n, len(lut), "first"), want, "first execute")
        shapes.same(shapes._read(ctx, r1, b1, W, n, len(lut), "index"), want, "execute_index in between")
        base._same(base._read_reply(ctx, r2, b2, W, n, len(lut), "second"), want, "second execute")
    finally:
        base._free_reply(ctx, r0, b0)
        shapes._free(ctx, r1, b1)
        base._free_reply(ctx, r2, b2)
        ctx.free(d_in)
        plan.close()


def _host_same(got, want, what):
    exp = indexref.expected_index(want)
    assert np.array_equal(got["index"], exp), what + ": index differs"
    assert np.array_equal(np.bincount(got["index"], minlength=len(want["c_hist"])), want["c_hist"]), what
    for k in ("gauge_mins", "gauge_maxs", "gauge_amps"):
        assert np.array_equal(got[k], want[k]), what + ": " + k
    assert np.array_equal(got["c_hist"].astype(np.int64), want["c_hist"]) and np.array_equal(got["cB_hist"].astype(np.int64), want["cB_hist"]), what
    assert np.array_equal(np.array([got["dBfs_min"], got["dBfs_max"]]).view(np.uint64),
                          np.array([want["dBfs_min"], want["dBfs_max"]], np.float64).view(np.uint64)), what


@pytest.mark.parametrize("wf", [False, True])
def test_render_index_dense_and_sparse(ctx, wf):
    n, fmt, lut = 256, "CS8", base._lut()
    win, weight = pyoracle.window("hann", n)
    for name, W, samples in (("dense", 45, n + 44 * 64), ("sparse", 48, n + 47 * 3 * n + 5)):
        data = siggen.generate(fmt, GEN, samples)
        want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf)
        got = ctx.render_index(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf, fill=0xAB)
        _host_same(got, want, name)
        if name == "sparse":
            assert ctx.last_upload_bytes() < data.size                 # the packed upload: the frames' own samples only
        else:
            assert ctx.last_upload_bytes() == data.size
    none = ctx.render_index(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf, want_index=False, fill=0xAB)
    assert (none["index"] == 0xAB).all() and np.array_equal(none["c_hist"].astype(np.int64), want["c_hist"])


@pytest.mark.parametrize("wf", [False, True])
def test_render_index_in_chunks(ctx, wf):
    """cu8, 2^25 samples, n = 1024, width 32768: 64 MiB of samples and a 32 MiB index image, which the streamer chunks."""
    n, fmt, W, lut = 1024, "CU8", 32768, base._lut()
    data = base._trinoise(fmt, 1 << 25)
    win, weight = pyoracle.window("hann", n)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf)
    got = ctx.render_index(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf, fill=0xAB)
    _host_same(got, want, "chunked wf=%d" % wf)
    assert ctx.last_chunks() >= 4, "the request was not chunked: %d chunk(s)" % ctx.last_chunks()
    assert ctx.last_upload_bytes() == data.size


# (the request, what it takes): 16 MiB of samples at width 1024 - the smallest request the streamer cuts - for every way through the
# host path that test_render_index_in_chunks does not take.  A peak request of one sub-frame per column is the sample detector's
# reply from k_frames, through the temporary RGBA image.
CHUNKED = {
    "packed frames_index": ("sample", 3, 2, "frames_index"),
    "contiguous render_extract": ("peak", 1, 1, "render_extract"),
    "packed render_extract": ("peak", 3, 2, "render_extract"),
}


@pytest.mark.parametrize("wf", [False, True])
@pytest.mark.parametrize("case", sorted(CHUNKED))
def test_render_index_in_chunks_every_path(ctx, case, wf):
    detector, num, den, kernel = CHUNKED[case]
    n, fmt, W, lut = 2048, "CF32", 1024, base._lut()
    data = siggen.generate(fmt, GEN, n + (W - 1) * n * num // den)
    assert W * n * 8 >= 16 << 20
    win, weight = pyoracle.window("hann", n)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut, False, wf, detector)
    try:
        assert plan.index_kernel_name_for(data.size, W) == kernel and plan.kernel_name(data.size, W) == "frames"
    finally:
        plan.close()
    got = ctx.render_index(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, wf, detector=detector, fill=0xAB)
    _host_same(got, want, "%s wf=%d" % (case, wf))
    assert ctx.last_chunks() > 1, "the request was not chunked"
    assert (ctx.last_upload_bytes() < data.size) == (num > den)


def test_render_index_of_a_peak_request_in_one_chunk(ctx):
    """sp_render_index through render_extract in one chunk: a peak request of three sub-frames per column."""
    n, fmt, W, lut = 128, "CU8", 37, base._lut()
    data, win, weight = _request(fmt, n, W, n + 36 * 3 * n + 19)
    want = peakref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, False, False)
    assert want["M"] == 3
    got = ctx.render_index(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, detector="peak", fill=0xAB)
    _host_same(got, want, "peak, one chunk")
    assert ctx.last_chunks() == 1 and ctx.last_upload_bytes() == data.size
