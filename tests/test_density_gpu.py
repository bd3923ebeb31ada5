"""The persistence spectrum on the device at the smallest shapes at which it can go wrong: sp_density_from_index on synthetic index
images, sp_plan_execute_density and sp_render_density against the oracle (tests/densityref.py), bit for bit.

The counts are integers, so there is no tolerance anywhere.  Output arrays start as garbage and lie between guard bytes; the widths of
the many-workgroups cases come from sp_debug_density_launch, so that several workgroups add to the same cells and the last is partial."""
import functools

import numpy as np
import pytest

import densityref
import peakref
import siggen
import test_index_launch_shapes_gpu as shapes
import test_launch_shapes_gpu as base
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GAIN, RANGE, GUARD = base.GAIN, base.RANGE, base.GUARD
pkg, ctx = base.pkg, base.ctx
GEN = {"kind": "trinoise", "seed": 5519, "step": 4099, "gshift": 9, "amp": 0.45, "namp": 0.03}


# ---- sp_density_from_index on images of the test's own -------------------------------------------------------------------------------

class _Counts:
    """A density array on the device between guard bytes, garbage (0xAB) at first."""

    def __init__(self, ctx, n, L, fill=0xAB):
        self.ctx, self.n, self.L, self.bytes = ctx, n, L, 4 * n * L
        self.blk = ctx.alloc(self.bytes + 2 * GUARD)
        ctx.memset(self.blk, fill, self.bytes + 2 * GUARD)
        self.fill = fill
        self.p = self.blk + GUARD

    def read(self, what):
        whole = self.ctx.download(self.blk, self.bytes + 2 * GUARD)
        assert (whole[:GUARD] == self.fill).all() and (whole[GUARD + self.bytes:] == self.fill).all(), what + ": bytes around the counts were written"
        return whole[GUARD:GUARD + self.bytes].view(np.uint32).reshape(self.n, self.L).copy()

    def free(self):
        self.ctx.free(self.blk)


def _count(ctx, image, n, W, wf, L, off=0, what=""):
    """sp_density_from_index of `image` placed `off` bytes past 16-byte alignment, into a garbage array."""
    d_ix = ctx.alloc(W * n + 32)
    out = _Counts(ctx, n, L)
    try:
        assert d_ix % 16 == 0
        if image.size:
            ctx.upload(d_ix + off, image)
        ctx.density_from_index(d_ix + off, n, W, wf, L, out.p)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_ix)
        out.free()


def _check(ctx, image, n, W, wf, L, off, what):
    got = _count(ctx, image, n, W, wf, L, off, what)
    want = densityref.count_image(image, n, W, wf, L)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d cells differ, first (row %d, index %d): %d, expected %d"
                             % (what, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])]))


# the issue's shapes, and two whose last band of rows is partial: spectrogram 8 + 1 rows over two passes of a lane, waterfall 64 + 36 bins
SHAPES = [(1, 1), (2, 1), (2, 5), (64, 15), (64, 16), (64, 17), (8, 4), (9, 700), (100, 33)]


@pytest.mark.parametrize("wf", [False, True])
@pytest.mark.parametrize("n,W", SHAPES)
def test_synthetic_images_every_alignment_and_map_length(ctx, n, W, wf):
    rng = np.random.default_rng(1000 * n + W)
    image = rng.integers(0, 256, n * W, dtype=np.uint8)
    for L in (1, 2, 255, 256):
        if L < 256 and n * W >= 600:
            assert (image >= L).any()                      # bytes the map does not have are present, and counted nowhere
        for off in (0, 1, 4):
            _check(ctx, image, n, W, wf, L, off, "n=%d W=%d wf=%d L=%d off=%d" % (n, W, wf, L, off))


@pytest.mark.parametrize("wf", [False, True])
def test_several_workgroups_add_to_one_row_and_the_last_is_partial(pkg, ctx, wf):
    n = 4
    frames = pkg.Library.get().debug_density_launch(n, 1 << 20, wf)["frames"]
    W = 3 * frames + 3
    d = pkg.Library.get().debug_density_launch(n, W, wf)
    assert d["pieces"] == 4 and d["bands"] == 1 and d["rects"][-1][3] - d["rects"][-1][2] == 3
    rng = np.random.default_rng(77 + wf)
    image = rng.integers(0, 7, n * W, dtype=np.uint8) * 41   # a few values: every workgroup hits every cell of its rows
    for off in (0, 1, 4):
        _check(ctx, image, n, W, wf, 256, off, "W=%d wf=%d off=%d" % (W, wf, off))
    _check(ctx, rng.integers(0, 256, n * W, dtype=np.uint8), n, W, wf, 200, 0, "W=%d wf=%d random" % (W, wf))


@pytest.mark.parametrize("wf", [False, True])
def test_flat_and_adversarial_images(ctx, wf):
    n, W, L = 16, 600, 200
    rng = np.random.default_rng(5)
    y, x = np.meshgrid(np.arange(n), np.arange(W), indexing="ij")
    rows = {"zeros": np.zeros((n, W), np.uint8), "last index": np.full((n, W), L - 1, np.uint8),
            "checkerboard": np.where((x + y) & 1, 3, 150).astype(np.uint8)}
    one = rng.integers(0, L, (n, W), dtype=np.uint8)
    one[5] = 17                                              # one flat row between random neighbours
    rows["one flat row"] = one
    for name, r in rows.items():
        image = r.reshape(-1) if not wf else np.ascontiguousarray(r.T[::-1, ::-1]).reshape(-1)   # [W - 1 - x][n - 1 - y]
        assert np.array_equal(densityref.rows_of(image, n, W, wf), r)
        _check(ctx, image, n, W, wf, L, 0, "%s wf=%d" % (name, wf))


def test_accumulate_overwrite_width_zero_and_refusals(pkg, ctx):
    n, W, L = 8, 50, 100
    image = np.random.default_rng(9).integers(0, 120, n * W, dtype=np.uint8)
    want = densityref.count_image(image, n, W, False, L)
    d_ix = ctx.alloc(W * n + 16)
    out = _Counts(ctx, n, L, fill=0xFF)
    try:
        ctx.upload(d_ix, image)
        ctx.density_from_index(d_ix, n, W, False, L, out.p)               # accumulate = 0 over 0xff: overwritten
        ctx.synchronize()
        assert np.array_equal(out.read("overwrite"), want)
        ctx.density_from_index(d_ix, n, W, False, L, out.p, accumulate=True)
        ctx.synchronize()
        assert np.array_equal(out.read("twice"), 2 * want)
        ctx.density_from_index(d_ix, n, 0, False, L, out.p, accumulate=True)   # width 0: nothing happens ...
        ctx.density_from_index(0, n, 0, False, L, out.p, accumulate=True)
        ctx.synchronize()
        assert np.array_equal(out.read("width 0, accumulate"), 2 * want)
        ctx.density_from_index(0, n, 0, False, L, out.p)                  # ... or the array is zeroed
        ctx.synchronize()
        assert (out.read("width 0") == 0).all()
        ctx.memset(out.p, 0xFF, 4 * n * L)
        ctx.density_from_index(d_ix, n, W, False, L, out.p, accumulate=True)   # 0xffffffff + count wraps modulo 2^32
        ctx.synchronize()
        assert np.array_equal(out.read("wrap"), (want.astype(np.int64) - 1).astype(np.uint32))
        ctx.memset(out.p, 0xFF, 4 * n * L)
        for bad in (dict(d_density=out.p + 1), dict(d_density=out.p + 2), dict(d_density=0), dict(lut_len=0), dict(lut_len=257),
                    dict(n=0), dict(width=-1), dict(d_index=0)):
            a = dict(dict(d_index=d_ix, n=n, width=W, waterfall=False, lut_len=L, d_density=out.p), **bad)
            with pytest.raises(pkg.SpectroplotError) as e:
                ctx.density_from_index(**a)
            assert e.value.status == -1, bad
        ctx.synchronize()
        assert (out.read("refused") == 0xFFFFFFFF).all()
    finally:
        ctx.free(d_ix)
        out.free()


# ---- requests against the oracle -----------------------------------------------------------------------------------------------------

def _data(fmt, samples, seed=0):
    return siggen.generate(fmt, dict(GEN, seed=GEN["seed"] + seed), samples)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(fmt, n, W, data, window, weight, channel mode, waterfall, detector, the oracle's reply): computed once, shared, left unchanged."""
    fmt, n, W, ch, wf, det, samples = {
        "cu8": ("CU8", 256, 300, False, False, "sample", 256 + 299 * 100 + 7),
        "cs16 lr waterfall": ("CS16", 256, 300, True, True, "sample", 256 + 299 * 70 + 3),
        "peak": ("CU8", 256, 37, False, False, "peak", 256 + 36 * 2 * 256 + 19),
        "n32": ("CS16", 32, 21, False, True, "sample", 32 + 20 * 16 + 1),
        "n2048": ("CS8", 2048, 70, False, False, "sample", 2048 + 69 * 300 + 5),
        "short": ("CU8", 64, 5, False, False, "sample", 40),
        "width 1": ("CU8", 64, 1, False, True, "sample", 200),
        "width 0": ("CU8", 64, 0, False, False, "sample", 200),
        "sparse": ("CS8", 256, 48, False, True, "sample", 256 + 47 * 3 * 256 + 5),
    }[name]
    data = _data(fmt, samples, len(name))
    win, weight = pyoracle.window("hann", n)
    lut = base._lut()
    if det == "peak":
        want = peakref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, ch, wf)
        assert want["M"] == 2
    else:
        want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, ch, wf)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    data.setflags(write=False)
    return fmt, n, W, data, win, weight, ch, wf, det, want


def _execute(ctx, plan, data, n, W, L, accumulate=False, what=""):
    d_in = ctx.alloc(data.size + 16)
    out = _Counts(ctx, n, L)
    try:
        ctx.upload(d_in, data)
        plan.execute_density(d_in, data.size, W, out.p, accumulate)
        ctx.synchronize()
        return out.read(what)
    finally:
        ctx.free(d_in)
        out.free()


def _assert_density(got, want, n, W, wf, c_hist, what):
    exp = densityref.expected(want, n, 256, W, wf)
    assert got.dtype == np.uint32 and got.shape == (n, 256), what
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError("%s: %d cells differ, first (row %d, index %d): %d, expected %d"
                             % (what, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], exp[tuple(bad[0])]))
    assert (got.sum(axis=1, dtype=np.int64) == W).all(), what + ": a row does not sum to the width"
    assert np.array_equal(got.sum(axis=0, dtype=np.int64), np.asarray(c_hist).astype(np.int64)), what + ": column sums are not sp_render's c_hist"


@pytest.mark.parametrize("name", ["cu8", "cs16 lr waterfall", "peak", "n32", "n2048", "short", "width 1", "width 0"])
def test_requests_against_the_oracle(ctx, name):
    fmt, n, W, data, win, weight, ch, wf, det, want = _case(name)
    lut = base._lut()
    c_hist = ctx.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, ch, wf, detector=det)["c_hist"]
    assert np.array_equal(c_hist.astype(np.int64), want["c_hist"])
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut, ch, wf, det)
    try:
        kernel = {"cu8": "frames_index", "cs16 lr waterfall": "frames_index", "n2048": "frames_index", "peak": "render_extract",
                  "n32": "render_extract"}.get(name)                     # both render paths are walked
        assert kernel is None or plan.index_kernel_name_for(data.size, W) == kernel
        _assert_density(_execute(ctx, plan, data, n, W, 256, what=name), want, n, W, wf, c_hist, name + ": execute_density")
    finally:
        plan.close()
    got = ctx.render_density(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, ch, wf, det, fill=0xABABABAB)
    _assert_density(got, want, n, W, wf, c_hist, name + ": render_density")
    if name == "short":
        assert (got[:, 0] == W).all() and (got[:, 1:] == 0).all()          # NaN frames: every count at index 0
    if name == "width 0":
        assert (got == 0).all()


def test_forced_scratch_kernel_counts_what_the_frame_loop_counts(ctx):
    fmt, n, W, data, win, weight, ch, wf, det, want = _case("cu8")
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, base._lut(), ch, wf, det)
    try:
        auto = _execute(ctx, plan, data, n, W, 256, what="auto")
        plan.force_kernel("scratch")
        assert plan.index_kernel_name_for(data.size, W) == "render_extract"
        forced = _execute(ctx, plan, data, n, W, 256, what="forced")
    finally:
        plan.close()
    assert np.array_equal(auto, forced)
    _assert_density(forced, want, n, W, wf, want["c_hist"], "forced to kernel 1")


def test_execute_density_accumulates_over_captures(ctx):
    """accumulate through the request path: a second capture's counts on top of the first's, on one array."""
    a, b = _case("cu8"), _case("sparse")
    lut = base._lut()
    out = _Counts(ctx, 256, 256)
    d_in = ctx.alloc(max(a[3].size, b[3].size) + 16)
    try:
        total = np.zeros((256, 256), np.int64)
        for k, (fmt, n, W, data, win, weight, ch, wf, det, want) in enumerate((a, b)):
            plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut, ch, wf, det)
            try:
                ctx.upload(d_in, data)
                plan.execute_density(d_in, data.size, W, out.p, accumulate=k > 0)
                ctx.synchronize()
            finally:
                plan.close()
            total += densityref.expected(want, n, 256, W, wf)
        assert np.array_equal(out.read("accumulated"), total.astype(np.uint32))
    finally:
        ctx.free(d_in)
        out.free()


# ---- the host path in chunks ---------------------------------------------------------------------------------------------------------

def test_chunked_host_path_and_sparse_upload(ctx):
    """cu8, n = 512, width 1100, a peak request of 16 sub-frames per column (a peak request travels whole): 18 MB of samples, which the
    streamer carries in chunks; every chunk's frames are rendered and counted behind its upload."""
    fmt, n, W, M, lut = "CU8", 512, 1100, 16, base._lut()
    data = siggen.generate(fmt, GEN, n + (W - 1) * M * n + 333)
    assert data.size >= 16 << 20 and W >= 1024                              # the documented threshold: the samples alone reach it
    win, weight = pyoracle.window("blackmanHarris", n)
    want = peakref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W)
    assert want["M"] == M
    got = ctx.render_density(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, detector="peak", fill=0xABABABAB)
    assert ctx.last_chunks() > 1, "the request was not chunked"
    assert ctx.last_upload_bytes() == data.size
    _assert_density(got, want, n, W, False, want["c_hist"], "chunked render_density")
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut, detector="peak")
    try:
        assert np.array_equal(_execute(ctx, plan, data, n, W, 256, what="unchunked"), got)
    finally:
        plan.close()
    # a sparse request of the sample detector: only the frames' own samples travel
    fmt, n, W, data, win, weight, ch, wf, det, want = _case("sparse")
    got = ctx.render_density(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, ch, wf, det, fill=0xABABABAB)
    assert ctx.last_upload_bytes() < data.size and ctx.last_chunks() == 1
    _assert_density(got, want, n, W, wf, want["c_hist"], "sparse render_density")


# (the request, what it takes): 16 MiB of samples at width 1024 - the smallest request the streamer cuts - for every way through the
# host path that the test above does not take.  A peak request of one sub-frame per column is the sample detector's reply from
# k_frames, through the temporary RGBA image.
CHUNKED = {
    "contiguous frames_index": ("sample", 1, 1, "frames_index"),
    "packed frames_index": ("sample", 3, 2, "frames_index"),
    "packed render_extract": ("peak", 3, 2, "render_extract"),
}


@pytest.mark.parametrize("case", sorted(CHUNKED))
def test_chunked_host_path_every_path(ctx, case):
    detector, num, den, kernel = CHUNKED[case]
    fmt, n, W, lut = "CF32", 2048, 1024, base._lut()
    data = siggen.generate(fmt, GEN, n + (W - 1) * n * num // den)
    assert W * n * 8 >= 16 << 20
    win, weight = pyoracle.window("hann", n)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut, detector=detector)
    try:
        assert plan.index_kernel_name_for(data.size, W) == kernel and plan.kernel_name(data.size, W) == "frames"
    finally:
        plan.close()
    got = ctx.render_density(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, W, detector=detector, fill=0xABABABAB)
    assert ctx.last_chunks() > 1, "the request was not chunked"
    assert (ctx.last_upload_bytes() < data.size) == (num > den)
    _assert_density(got, want, n, W, False, want["c_hist"], case)


# ---- one context, no synchronisation in between --------------------------------------------------------------------------------------

def test_density_rgba_index_density_interleave_without_a_sync(ctx):
    fmt, n, W, data, win, weight, ch, wf, det, want = _case("cu8")
    lut = base._lut()
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, lut)
    d_in = ctx.alloc(data.size + 16)
    c0, c3 = _Counts(ctx, n, 256), _Counts(ctx, n, 256)
    r1, b1 = base._alloc_reply(ctx, W, n, 256, False)
    r2, b2 = shapes._alloc(ctx, W, n, 256, 0)
    try:
        ctx.upload(d_in, data)
        plan.execute_density(d_in, data.size, W, c0.p)
        plan.execute(d_in, data.size, W, **r1)
        plan.execute_index(d_in, data.size, W, **r2)
        plan.execute_density(d_in, data.size, W, c3.p)
        ctx.synchronize()
        _assert_density(c0.read("first"), want, n, W, wf, want["c_hist"], "first execute_density")
        base._same(base._read_reply(ctx, r1, b1, W, n, 256, "rgba"), want, "execute in between")
        shapes.same(shapes._read(ctx, r2, b2, W, n, 256, "index"), want, "execute_index in between")
        _assert_density(c3.read("last"), want, n, W, wf, want["c_hist"], "last execute_density")
    finally:
        base._free_reply(ctx, r1, b1)
        shapes._free(ctx, r2, b2)
        c0.free()
        c3.free()
        ctx.free(d_in)
        plan.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(pkg, ctx):
    import ctypes as C
    fmt, n, W = "CU8", 64, 8
    data = _data(fmt, 64 * 8)
    win, weight = pyoracle.window("hann", n)
    i = np.arange(257)
    long_lut = np.stack([i & 255, i >> 8, i & 255], axis=1).astype(np.uint8)
    d_in = ctx.alloc(data.size + 16)
    out = _Counts(ctx, n, 257)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, long_lut)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            plan.execute_density(d_in, data.size, W, out.p)
        assert e.value.status == -4                                   # SP_ERR_UNSUPPORTED: a byte cannot hold the index
        with pytest.raises(pkg.SpectroplotError) as e:
            ctx.render_density(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, long_lut, W)
        assert e.value.status == -4
    finally:
        plan.close()
    plan = ctx.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, base._lut())
    try:
        for bad in (dict(d_density=out.p + 2), dict(d_density=0), dict(width=-1)):
            a = dict(dict(d_bytes=d_in, nbytes=data.size, width=W, d_density=out.p), **bad)
            with pytest.raises(pkg.SpectroplotError) as e:
                plan.execute_density(**a)
            assert e.value.status == -1, bad
        ctx.synchronize()
        assert (out.read("refused") == 0xABABABAB).all()
    finally:
        plan.close()
        ctx.free(d_in)
        out.free()
    L = pkg.Library.get().L                                            # no plan, no context: what sp_plan_execute_index answers
    assert L.sp_plan_execute_density(None, None, 0, 0, None, 0) == L.sp_plan_execute_index(None, None, 0, 0, None, None) == -1
    assert L.sp_render_density(None, None, None, 0, 0, None) == L.sp_render_index(None, None, None, 0, 0, None, None) == -1
    assert L.sp_density_from_index(None, None, 1, 0, 0, 1, None, 0) == L.sp_index_to_rgba(None, None, 0, None, 0, None) == -1
    assert C.sizeof(pkg.binding._Request) == 64


def _hip_runtime(pkg):
    """The HIP runtime the library itself is linked to and has loaded, through ctypes (a second copy would know nothing of its streams)."""
    import ctypes as C
    pkg.Library.get()
    paths = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln]
    assert paths, "the library has not loaded a HIP runtime"
    own = [p for p in paths if "torch" not in p] or paths
    return C.CDLL(own[0])


def test_a_capturing_stream_refuses_the_request_and_takes_the_count(pkg):
    """sp_plan_execute_density carries a request number (SP_ERR_UNSUPPORTED on a capturing stream); sp_density_from_index does not and is
    captured.  The capture is ended and the graph discarded: nothing is replayed."""
    import ctypes as C
    hip = _hip_runtime(pkg)
    fmt, n, W = "CU8", 64, 24
    data = _data(fmt, 64 * 30)
    win, weight = pyoracle.window("hann", n)
    image = np.random.default_rng(3).integers(0, 256, n * W, dtype=np.uint8)
    own = pkg.Context(0)
    stream, graph = C.c_void_p(), C.c_void_p()
    try:
        plan = own.plan(fmt, n, win, 1.0 / weight, GAIN, RANGE, base._lut())
        d_in, d_ix = own.alloc(data.size + 16), own.alloc(n * W)
        out = _Counts(own, n, 256)
        own.upload(d_in, data)
        own.upload(d_ix, image)
        assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
        own.set_stream(stream.value)
        plan.execute_density(d_in, data.size, W, out.p)                # (outside a capture: accepted; the workspaces exist from here on)
        own.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0               # hipStreamCaptureModeThreadLocal
        try:
            with pytest.raises(pkg.SpectroplotError) as e:
                plan.execute_density(d_in, data.size, W, out.p)
            own.density_from_index(d_ix, n, W, False, 256, out.p)      # accepted: recorded, not run
        finally:
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
            if graph.value:
                assert hip.hipGraphDestroy(graph) == 0                 # discarded: nothing is replayed
        assert e.value.status == -4
        own.synchronize()
        own.density_from_index(d_ix, n, W, False, 256, out.p)          # the context works on after the capture
        own.synchronize()
        assert np.array_equal(out.read("after the capture"), densityref.count_image(image, n, W, False, 256))
        plan.close()
        for p in (d_in, d_ix):
            own.free(p)
        out.free()
    finally:
        own.set_stream(None)
        own.close()
        if stream.value:
            hip.hipStreamDestroy(stream)
