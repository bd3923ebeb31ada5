"""Power plane replies on the GPU (sp_plan_execute_power, sp_plan_power_to_db, sp_render_power): every value compared bit for bit with
the oracle's abs2 / db planes in row order (tests/powerref.py; which NaN a NaN is, is the one thing left uncompared), through both
frame loops (k_frames_power and the portable k_scratch_power) and both entry points.  Every device plane lies between guard bytes, and
plane and guards hold garbage before the call.

The measurement that goes with the feature is not asserted here (tools/power_bench.py)."""
import ctypes as C

import numpy as np
import pytest

import launchref
import powerref
import siggen
import tracesref
from __graft_entry__ import load_package
from oracle import pyoracle
from peakref import _clamp_u8
from test_gpu_parity import FROM_HOST, _assert_same as assert_same_reply

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 27182, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
GARBAGE = 0xAB
GUARD = 4096
FRAME_SIZES = [64, 128, 256, 512, 1024]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Plane:
    """A device plane f64 [width, n] between two guards, everything garbage."""

    def __init__(self, ctx, width, n):
        self.ctx, self.width, self.n, self.size = ctx, width, n, 8 * width * n
        self.base = ctx.alloc(self.size + 2 * GUARD)
        assert self.base % 8 == 0
        self.ptr = self.base + GUARD
        self.fill()

    def fill(self):
        self.ctx.memset(self.base, GARBAGE, self.size + 2 * GUARD)

    def read(self, what=""):
        whole = self.ctx.download(self.base, self.size + 2 * GUARD)
        assert (whole[:GUARD] == GARBAGE).all() and (whole[GUARD + self.size:] == GARBAGE).all(), what + ": bytes around the plane were written"
        return whole[GUARD:GUARD + self.size].view(np.float64).reshape(self.width, self.n)

    def free(self):
        self.ctx.free(self.base)


def _upload(ctx, data):
    d_in = ctx.alloc(max(data.size, 16))
    if data.size:
        ctx.upload(d_in, data)
    return d_in


def _execute(ctx, plan, d_in, nbytes, width, n, what, db=None):
    """sp_plan_execute_power into a guarded garbage plane; db: None, "out" (a second guarded plane) or "in" (in place)."""
    pl = _Plane(ctx, width, n)
    other = _Plane(ctx, width, n) if db == "out" else None
    try:
        plan.execute_power(d_in, nbytes, width, pl.ptr)
        if db == "out":
            plan.power_to_db(pl.ptr, width * n, other.ptr)
        elif db == "in":
            plan.power_to_db(pl.ptr, width * n, pl.ptr)
        ctx.synchronize()
        got = pl.read(what)
        return (got, other.read(what + " (dB)")) if other else got
    finally:
        pl.free()
        if other:
            other.free()


def _check_case(ctx, fmt, n, width, data, ch=False, main=True, window="hann", gain=3.0, rng=50.0, win=None, host=True):
    """Reference once; sp_plan_execute_power automatically, forced onto the portable kernel, automatically again; the dB plane out of
    place; sp_render_power both ways.  Returns the expected planes."""
    if win is None:
        win, weight = pyoracle.window(window, n)
        bn = 1.0 / weight
    else:
        bn = 1.0 / n
    what = "%s n=%d W=%d%s" % (fmt, n, width, " L/R" if ch else "")
    want = powerref.expected(fmt, data, n, win, bn, gain, rng, width, ch)
    if main:
        powerref.assert_telling(want["power"], what)
    plan = ctx.plan(fmt, n, win, bn, gain, rng, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        covered = n in FRAME_SIZES and np.isfinite(win).all()
        name = "frames_power" if covered else "scratch_power"
        assert plan.power_kernel_name_for(data.size, width) == name
        auto = _execute(ctx, plan, d_in, data.size, width, n, what + " automatic")
        powerref.assert_same(auto, want["power"], what + " automatic")
        plan.force_kernel("scratch")
        assert plan.power_kernel_name_for(data.size, width) == "scratch_power"
        portable = _execute(ctx, plan, d_in, data.size, width, n, what + " portable")
        powerref.assert_same(portable, want["power"], what + " portable")
        try:
            plan.force_kernel("frames")          # (refused where k_frames does not cover the plan's renders: the force stays)
        except Exception as e:
            assert getattr(e, "status", None) == -4
        plan.force_kernel("auto")
        assert plan.power_kernel_name_for(data.size, width) == name
        again, db = _execute(ctx, plan, d_in, data.size, width, n, what + " automatic again", db="out")
        powerref.assert_same(again, want["power"], what + " automatic again")
        assert powerref.same_plane(auto, portable) and powerref.same_plane(auto, again)
        powerref.assert_same(db, want["db"], what + " power_to_db")
    finally:
        ctx.free(d_in)
        plan.close()
    if host:
        got = ctx.render_power(fmt, data, n, win, bn, gain, rng, width, ch, fill=GARBAGE)
        powerref.assert_same(got, want["power"], what + " sp_render_power")
        got = ctx.render_power(fmt, data, n, win, bn, gain, rng, width, ch, db=True, fill=GARBAGE)
        powerref.assert_same(got, want["db"], what + " sp_render_power db")
    return want


def _capture(fmt, n, width, stride_num, stride_den=1, extra=0):
    """A capture whose stride is stride_num / stride_den samples (exactly, for width >= 2)."""
    samples = n + (max(width, 1) - 1) * stride_num // stride_den + extra
    return siggen.generate(fmt, GEN, samples)


# ---- (a) every size of the frame loop at widths of a few groups with a ragged last group, (b) the portable kernel's own sizes ------------
@pytest.mark.parametrize("n,width", [(64, 700), (128, 333), (256, 150), (512, 77), (1024, 41)])
def test_frame_loop_sizes(ctx, n, width):
    _check_case(ctx, "CS16", n, width, _capture("CS16", n, width, n // 2 + 3))


@pytest.mark.parametrize("n,width", [(2, 64), (16, 64), (32, 33), (2048, 17), (8192, 5)])
def test_portable_kernel_sizes(ctx, n, width):
    # (the hann taper of two points is all zeros)
    _check_case(ctx, "CS16", n, width, _capture("CS16", n, width, n // 2 + 3), window="blackmanHarris" if n == 2 else "hann")


def test_non_finite_taper_takes_the_portable_kernel(ctx):
    n, width = 256, 20
    win = pyoracle.window("hann", n)[0].copy()
    win[17] = np.inf
    want = _check_case(ctx, "CS16", n, width, _capture("CS16", n, width, n), main=False, win=win)
    assert np.isnan(want["power"]).any() or np.isinf(want["power"]).any()


# ---- (c) launch regimes ----------------------------------------------------------------------------------------------------------------
SHAPE_FORMATS = ["CS16", "CU8", "CF32", "CS12", "CU4"]
REGIME_SHIFT = {"one": 2, "mixed": 0, "many": 1}


@pytest.mark.parametrize("regime", ["one", "mixed", "many"])
@pytest.mark.parametrize("n", FRAME_SIZES)
def test_launch_shapes(pkg, ctx, n, regime):
    """Fewer groups than workgroups (smallest gf), some workgroups with two groups and some with one (smallest gf), three groups or more
    for every workgroup (largest gf: rounds > 1, the HALVES slot mapping at n = 1024); always a ragged last group - whose slots past the
    end must store nothing - and a group count that is no multiple of 8."""
    k = FRAME_SIZES.index(n)
    fmt, ch = SHAPE_FORMATS[(k + REGIME_SHIFT[regime]) % 5], (k + (regime == "mixed")) % 2 == 1
    win, weight = pyoracle.window("hann", n)
    probe = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, ch)
    cu = probe.debug_launch(16 * n, 4)["cu_count"]
    probe.close()
    gfs = launchref.reachable_gf(n)
    gf = gfs[-1] if regime == "many" else gfs[0]
    width = launchref.choose_width(n, cu, gf, regime, w4=False)
    assert width is not None
    gf_l, groups, grid, _ = pkg.binding.debug_frames_launch(n, 2, width, cu)          # the rule k_frames_power launches by
    assert gf_l == gf and groups % 8 != 0 and width % gf != 0 and launchref.regime_of(groups, grid) == regime
    assert launchref.halves(n, gf) == (n == 1024 and regime == "many")
    assert width * n * 8 < 1 << 30
    data = siggen.generate(fmt, GEN, n + (width - 1) * 67 + 29)                            # a fractional stride of about 67 samples
    want = _check_case(ctx, fmt, n, width, data, ch=ch, main=not ch, host=False)
    if ch:
        assert (want["power"][:, 0] == 0.0).all() and not np.signbit(want["power"][:, 0]).any()
        powerref.assert_telling(want["power"][:, 1:])



@pytest.mark.parametrize("n,width", [(64, 3), (256, 5), (1024, 2)])
def test_fewer_frames_than_slots(ctx, n, width):
    """One group that does not fill a round: most slots of the workgroup have no frame at all."""
    assert width < launchref.THREADS * 16 // n
    _check_case(ctx, "CS16", n, width, _capture("CS16", n, width, n + 5))


# ---- (d) every loader ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("fmt", ["CU4", "CS8", "CS12", "CU12", "CU16", "CS32", "CF32", "CF64", "CU64"])
def test_every_loader(ctx, fmt, n):
    width = 45
    _check_case(ctx, fmt, n, width, _capture(fmt, n, width, n + 7))


# ---- (e) L/R split ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width", [("CS16", 64, 300), ("CF32", 256, 90), ("CU8", 512, 50), ("CF32", 1024, 37), ("CS12", 2048, 12)])
def test_channel_mode(ctx, fmt, n, width):
    want = _check_case(ctx, fmt, n, width, _capture(fmt, n, width, n // 3 + 1), ch=True, main=False)
    # the split forces bin n/2 to zero: row 0 is exactly +0.0 and -inf in dB; every other row is telling
    assert (want["power"][:, 0].view(np.uint64) == 0).all() and (want["db"][:, 0] == -np.inf).all()
    powerref.assert_telling(want["power"][:, 1:])


# ---- (f) edge shapes (reference NaNs allowed, compared by position) ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [128, 1024, 4096])
def test_fractional_stride_overlap_and_sparse(ctx, n):
    _check_case(ctx, "CU8", n, 37, siggen.generate("CU8", GEN, n + 36 * n + 17))          # fractional, just above n
    _check_case(ctx, "CU8", n, 50, _capture("CU8", n, 50, n // 5))                        # stride < n
    _check_case(ctx, "CS16", n, 23, _capture("CS16", n, 23, 2 * n + 5, extra=3))          # stride >= 2 n, fractional


@pytest.mark.parametrize("n", [64, 1024, 2048])
def test_width_zero_and_one(pkg, ctx, n):
    data = siggen.generate("CS16", GEN, 3 * n)
    _check_case(ctx, "CS16", n, 1, data)
    _check_case(ctx, "CS16", n, 0, data, main=False)
    _check_case(ctx, "CS16", n, 0, np.zeros(0, np.uint8), main=False)                     # ... and no capture at all
    # width 0 writes nothing: a plane of one frame and its guards are still garbage, and a NULL plane is accepted
    win, weight = pyoracle.window("hann", n)
    plan = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    pl = _Plane(ctx, 1, n)
    d_in = _upload(ctx, data)
    try:
        plan.execute_power(d_in, data.size, 0, pl.ptr)
        plan.execute_power(d_in, data.size, 0, 0)
        plan.power_to_db(pl.ptr, 0, pl.ptr)
        ctx.synchronize()
        assert (pl.read("width 0").view(np.uint8) == GARBAGE).all()
    finally:
        pl.free()
        ctx.free(d_in)
        plan.close()


@pytest.mark.parametrize("n", [64, 1024, 2048])
def test_capture_shorter_than_n(ctx, n):
    data = siggen.generate("CS16", GEN, n // 2 + 3)
    want = _check_case(ctx, "CS16", n, 3, data, main=False)
    assert np.isnan(want["power"]).all()


@pytest.mark.parametrize("n", [256, 1024, 2048])
def test_last_frame_ends_past_the_capture(ctx, n):
    """An odd byte count of CU8: the last frame starts half a sample late and reads one sample past the typed view (undefined -> NaN in
    the reference): not in bounds, the generic loaders."""
    width = 40
    data = siggen.generate("CU8", GEN, n + 39 * (n // 2))
    data = np.concatenate([data, np.array([77], np.uint8)])
    want = _check_case(ctx, "CU8", n, width, data, main=False)
    assert np.isnan(want["power"][-1]).all()
    powerref.assert_telling(want["power"][:-1])


@pytest.mark.parametrize("n", [128, 1024, 2048])
def test_nan_and_infinite_samples(ctx, n):
    width = 30
    data = siggen.generate("CF32", GEN, n + 29 * (n + 3))
    f = data.view("<f4").reshape(-1, 2)
    f[3 * (n + 3) + 7, 0] = np.nan
    f[7 * (n + 3) + n - 1, 1] = np.nan
    f[11 * (n + 3) + 1, 0] = np.inf
    f[12 * (n + 3) + n // 2, 1] = -np.inf
    want = _check_case(ctx, "CF32", n, width, data, main=False)
    assert np.isnan(want["power"]).any() and (want["power"] == np.inf).any() and np.isfinite(want["power"][0]).all()


@pytest.mark.parametrize("fmt,n", [("CS16", 64), ("CF32", 1024), ("CS8", 4096)])
def test_all_zero_capture(ctx, fmt, n):
    width = 19
    data = np.zeros(siggen.SAMPLE_WIDTH[fmt] * (n + 18 * (n + 1)), np.uint8)
    want = _check_case(ctx, fmt, n, width, data, main=False)
    assert (want["power"].view(np.uint64) == 0).all() and (want["db"] == -np.inf).all()          # every value +0.0


# ---- (g) power_to_db -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [3.0, 0.1])
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 256, 70, False), ("CF32", 1024, 21, True), ("CU8", 2048, 9, False)])
def test_power_to_db_in_and_out_of_place(ctx, fmt, n, width, ch, gain):
    data = _capture(fmt, n, width, n + n // 4 + 1)
    win, weight = pyoracle.window("blackmanHarris", n)
    want = powerref.expected(fmt, data, n, win, 1.0 / weight, gain, 40.0, width, ch)
    powerref.assert_telling(want["db"][:, 1:] if ch else want["db"])
    if ch:
        assert (want["db"][:, 0] == -np.inf).all()
    plan = ctx.plan(fmt, n, win, 1.0 / weight, gain, 40.0, powerref._LUT, ch)
    d_in = _upload(ctx, data)
    try:
        power, db = _execute(ctx, plan, d_in, data.size, width, n, "out of place", db="out")
        powerref.assert_same(power, want["power"], "the source of an out-of-place conversion")
        powerref.assert_same(db, want["db"], "out of place")
        powerref.assert_same(_execute(ctx, plan, d_in, data.size, width, n, "in place", db="in"), want["db"], "in place")
    finally:
        ctx.free(d_in)
        plan.close()


# ---- (h) invariants with the other replies ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width,ch", [("CS16", 512, 130, False), ("CF32", 1024, 70, True), ("CU8", 2048, 20, False)])
def test_db_plane_folds_to_the_traces_and_the_gauges(ctx, fmt, n, width, ch):
    gain, rng = 6.0, 40.0
    data = _capture(fmt, n, width, n + n // 4 + 1)
    win, weight = pyoracle.window("blackmanHarris", n)
    lut = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, gain, rng, lut, ch)
    d_in = _upload(ctx, data)
    d_tr = ctx.alloc(16 * n)
    try:
        db = _execute(ctx, plan, d_in, data.size, width, n, "dB plane", db="in")
        plan.execute_traces(d_in, data.size, width, d_tr, d_tr + 8 * n)
        ctx.synchronize()
        tr = ctx.download(d_tr, 16 * n, np.float64)
    finally:
        ctx.free(d_in)
        ctx.free(d_tr)
        plan.close()
    tmin, tmax = tracesref.fold(db)                      # (min / max over x with the start values 0, -200)
    assert tracesref.same_bits(tmin, tr[:n]) and tracesref.same_bits(tmax, tr[n:])
    reply = ctx.render(fmt, data, n, win, 1.0 / weight, gain, rng, lut, width, ch)
    with np.errstate(all="ignore"):
        fmin = np.fmin(np.fmin.reduce(db, axis=1), 0.0)                                    # worker.js:102-103
        fmax = np.fmax(np.fmax.reduce(db, axis=1), -200.0)
        assert np.array_equal(_clamp_u8(0.5 + (rng + fmin) * 256 / rng), reply["gauge_mins"])      # worker.js:126-129
        assert np.array_equal(_clamp_u8(0.5 + (rng + fmax) * 256 / rng), reply["gauge_maxs"])
    assert len(np.unique(reply["gauge_maxs"])) > 1 or len(np.unique(reply["gauge_mins"])) > 1


# ---- (i) the host entry point ------------------------------------------------------------------------------------------------------------------
def test_small_sparse_request_uploads_its_frames_only(ctx):
    fmt, n, width = "CU8", 256, 64
    data = _capture(fmt, n, width, 40 * n + 11)
    _check_case(ctx, fmt, n, width, data)
    assert ctx.last_upload_bytes() < data.size // 8 and ctx.last_chunks() == 1


def _device_planes(ctx, fmt, n, width, data, win, bn, gain=3.0, rng=50.0):
    plan = ctx.plan(fmt, n, win, bn, gain, rng, powerref._LUT)
    d_in = _upload(ctx, data)
    try:
        return _execute(ctx, plan, d_in, data.size, width, n, "device planes", db="out")
    finally:
        ctx.free(d_in)
        plan.close()


CHUNKED = ("CU8", 64, 32768)          # 16 MiB of plane: the smallest request the streamer cuts


@pytest.fixture(scope="module")
def chunked(ctx):
    fmt, n, width = CHUNKED
    data = _capture(fmt, n, width, n // 2 + 1)
    assert 8 * width * n >= 16 << 20
    win, weight = pyoracle.window("hann", n)
    want = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width)
    powerref.assert_telling(want["power"], "chunked")
    return data, win, 1.0 / weight, want


@pytest.mark.parametrize("db", [False, True])
def test_chunked_sp_render_power(ctx, chunked, db):
    fmt, n, width = CHUNKED
    data, win, bn, want = chunked
    got = ctx.render_power(fmt, data, n, win, bn, 3.0, 50.0, width, db=db, fill=GARBAGE)
    assert ctx.last_chunks() > 1 and ctx.last_upload_bytes() == data.size
    powerref.assert_same(got, want["db" if db else "power"], "chunked, db=%r" % db)


def test_chunked_sp_render_power_waits_for_a_queued_execute_from_host(pkg, ctx, chunked):
    """sp_plan_execute_from_host returns with its copies and kernels still queued on the context's staging buffer; a chunked
    sp_render_power on the same context, called WITHOUT a synchronisation in between, must not upload over them."""
    r_fmt, r_n, r_lg, W, r_wf = FROM_HOST[3]                  # sparse, one packed chunk: it shares the staging buffer's first bytes
    r_data = siggen.generate(r_fmt, {"kind": "trinoise", "seed": 99 + r_n, "step": 7321, "gshift": 9, "amp": 0.5, "namp": 0.02}, 1 << r_lg)
    r_win, r_weight = pyoracle.window("blackmanHarris", r_n)
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    r_want = pyoracle.render(r_fmt, r_data, r_n, r_win, 1.0 / r_weight, 6.0, 30.0, lut, W, False, r_wf)
    fmt, n, width = CHUNKED
    data, win, bn, want = chunked
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
        # once before, so that nothing between the two calls below synchronises by itself (the plane's plan, staging buffers, streams)
        powerref.assert_same(ctx.render_power(fmt, data, n, win, bn, 3.0, 50.0, width, fill=GARBAGE), want["power"], "before")
        for p_, s_ in zip(ptrs, sizes):
            ctx.memset(p_, 0xA5, max(s_, 16))
        for _ in range(16):                                    # a few ms of work ahead of the request on the context's stream
            ctx.memset(busy, 0, 1 << 30)
        plan.execute_from_host(pinned, W, *ptrs)
        got = ctx.render_power(fmt, data, n, win, bn, 3.0, 50.0, width, fill=GARBAGE)
        ctx.synchronize()
        assert ctx.last_chunks() > 1
        r_got = {"rgba": ctx.download(ptrs[0], sizes[0]), "gauge_mins": ctx.download(ptrs[1], W), "gauge_maxs": ctx.download(ptrs[2], W),
                 "gauge_amps": ctx.download(ptrs[3], W), "c_hist": ctx.download(ptrs[4], 8 * 256, np.uint64),
                 "cB_hist": ctx.download(ptrs[5], 8000, np.uint64)}
        mm = ctx.download(ptrs[6], 16, np.float64)
        r_got["dBfs_min"], r_got["dBfs_max"] = float(mm[0]), float(mm[1])
        assert_same_reply(r_got, r_want)
        powerref.assert_same(got, want["power"], "behind a queued execute_from_host")
    finally:
        L.sp_host_free(h)
        for p_ in ptrs + [busy]:
            ctx.free(p_)
        plan.close()


# ---- (j) interleaving ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,n,width", [("CS16", 256, 333), ("CU8", 2048, 21)])
def test_execute_power_and_index_interleave_without_a_synchronisation(ctx, fmt, n, width):
    data = _capture(fmt, n, width, n // 2 + 3)
    win, weight = pyoracle.window("hann", n)
    i = np.arange(256)
    lut = np.stack([i, 255 - i, (i * 7) & 255], axis=1).astype(np.uint8)
    ident = np.stack([i, i * 0, i * 0], axis=1).astype(np.uint8)
    want = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width)
    powerref.assert_telling(want["power"])
    r_want = pyoracle.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width)
    i_want = pyoracle.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, ident, width)["rgba"][0::4]
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, lut)
    d_in = _upload(ctx, data)
    sizes = [4 * width * n, width, width, width, 8 * 256, 8000, 16]
    ptrs = [ctx.alloc(s_) for s_ in sizes]
    d_index = ctx.alloc(width * n)
    pl = _Plane(ctx, width, n)
    try:
        for p_, s_ in zip(ptrs, sizes):
            ctx.memset(p_, 0xA5, s_)
        ctx.memset(d_index, 0xA5, width * n)
        ctx.synchronize()
        plan.execute(d_in, data.size, width, *ptrs)
        plan.execute_power(d_in, data.size, width, pl.ptr)
        plan.execute_index(d_in, data.size, width, d_index)
        ctx.synchronize()
        r_got = {"rgba": ctx.download(ptrs[0], sizes[0]), "gauge_mins": ctx.download(ptrs[1], width), "gauge_maxs": ctx.download(ptrs[2], width),
                 "gauge_amps": ctx.download(ptrs[3], width), "c_hist": ctx.download(ptrs[4], 8 * 256, np.uint64),
                 "cB_hist": ctx.download(ptrs[5], 8000, np.uint64)}
        mm = ctx.download(ptrs[6], 16, np.float64)
        r_got["dBfs_min"], r_got["dBfs_max"] = float(mm[0]), float(mm[1])
        assert_same_reply(r_got, r_want)
        powerref.assert_same(pl.read("interleaved"), want["power"], "interleaved")
        assert np.array_equal(ctx.download(d_index, width * n), i_want)
    finally:
        pl.free()
        for p_ in ptrs + [d_index, d_in]:
            ctx.free(p_)
        plan.close()


# ---- (k) refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    n, width = 128, 20
    data = _capture("CU8", n, width, 3 * n)
    win, weight = pyoracle.window("hann", n)
    L = ctx.lib.L
    d_in, d_out = ctx.alloc(data.size), ctx.alloc(8 * width * n + 16)
    vp = C.c_void_p
    peak = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
    plan = ctx.plan("CU8", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            peak.execute_power(d_in, data.size, width, d_out)
        assert e.value.status == -4 and "peak" in str(e.value)
        assert L.sp_plan_execute_power(None, vp(d_in), data.size, width, vp(d_out)) == -1
        assert L.sp_plan_execute_power(plan.h, vp(d_in), data.size, width, vp(d_out + 4)) == -1      # misaligned
        assert L.sp_plan_execute_power(plan.h, vp(d_in), data.size, width, None) == -1               # NULL
        # check_capture's own statuses
        assert L.sp_plan_execute_power(plan.h, vp(d_in), data.size, -1, vp(d_out)) == -1
        assert L.sp_plan_execute_power(plan.h, None, data.size, width, vp(d_out)) == -1
        plan16 = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
        assert L.sp_plan_execute_power(plan16.h, vp(d_in), 4 * 100 + 1, width, vp(d_out)) == -3
        plan16.close()
        assert L.sp_plan_power_to_db(None, vp(d_out), 8, vp(d_out)) == -1
        assert L.sp_plan_power_to_db(plan.h, vp(d_out + 4), 8, vp(d_out)) == -1
        assert L.sp_plan_power_to_db(plan.h, vp(d_out), 8, vp(d_out + 2)) == -1
        assert L.sp_plan_power_to_db(plan.h, None, 8, vp(d_out)) == -1
        assert L.sp_plan_power_to_db(plan.h, vp(d_out), 0, vp(d_out)) == 0
        assert L.sp_plan_power_kernel_name_for(None, 0, 0) == b""
        ctx.synchronize()
    finally:
        peak.close()
        plan.close()
        ctx.free(d_in)
        ctx.free(d_out)
    req, keep = pkg.binding._make_request(pkg.parse_format("CU8")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False, "peak")
    out = np.zeros(width * n)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    assert L.sp_render_power(ctx.h, C.byref(req), p(data), data.size, width, 0, p(out)) == -4
    req.detector = 0
    assert L.sp_render_power(None, C.byref(req), p(data), data.size, width, 0, p(out)) == -1
    assert L.sp_render_power(ctx.h, None, p(data), data.size, width, 0, p(out)) == -1
    assert L.sp_render_power(ctx.h, C.byref(req), None, data.size, width, 0, p(out)) == -1
    assert L.sp_render_power(ctx.h, C.byref(req), p(data), data.size, -2, 0, p(out)) == -1
    assert L.sp_render_power(ctx.h, C.byref(req), p(data), data.size, width, 0, None) == -1
    assert L.sp_render_power(ctx.h, C.byref(req), p(data), data.size, width, 0, vp(out.ctypes.data + 4)) == -1
    req16, keep16 = pkg.binding._make_request(pkg.parse_format("CS16")[0], n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, False, False)
    assert L.sp_render_power(ctx.h, C.byref(req16), p(data), 4 * 100 + 1, width, 0, p(out)) == -3
    assert L.sp_render_power(ctx.h, C.byref(req), p(data), data.size, width, 0, p(out)) == 0
