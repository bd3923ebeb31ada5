"""The peak detector on the GPU: every reply field compared exactly with the expected values tests/peakref.py builds from the oracle,
through both kernels (k_frames_peak and the portable scratch kernel) and every entry point that takes the detector.

The measurement that goes with the detector is not asserted here (tools/peak_bench.py): the peak render at 2 048
columns against the sample render at 2 048 * M columns meets "no slower, 5 % margin" at n = 1024 (0.73-0.87) and misses it at n = 512
(1.18-1.28: 2 048 columns are 128 workgroups on 256 CUs; at 4 096 columns the same kernel measures 0.70-0.80)."""
import numpy as np
import pytest

import peakref
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 31337, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _lut(L=256):
    lut = np.stack([np.arange(L) & 255, (np.arange(L)[::-1]) & 255, (np.arange(L) * 3) & 255], axis=1).astype(np.uint8)
    lut[0] = 0
    lut[-1] = 255
    return lut


def _samples(n, width, M, extra):
    """A capture length whose stride is M * n + extra / (width - 1): M sub-frames per column."""
    return n + (width - 1) * M * n + extra


def _execute(ctx, plan, data, width, n, L, from_host=False):
    """sp_plan_execute (or _from_host) on device buffers; the reply as numpy arrays."""
    W = max(int(width), 0)
    sizes = {"rgba": 4 * W * n, "gauge_mins": W, "gauge_maxs": W, "gauge_amps": W, "c_hist": 8 * L, "cb_hist": 8000, "dbfs_minmax": 16}
    ptrs = {k: ctx.alloc(max(v, 16)) for k, v in sizes.items()}
    d_in = ctx.alloc(max(data.size, 16))
    try:
        for k, v in sizes.items():
            ctx.memset(ptrs[k], 0xAB, max(v, 16))
        if from_host:
            plan.execute_from_host(data, width, **ptrs)
        else:
            ctx.upload(d_in, data)
            plan.execute(d_in, data.size, width, **ptrs)
        ctx.synchronize()
        out = {k: ctx.download(ptrs[k], sizes[k]) for k in ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps")}
        out["c_hist"] = ctx.download(ptrs["c_hist"], 8 * L, np.uint64)
        out["cB_hist"] = ctx.download(ptrs["cb_hist"], 8000, np.uint64)
        mm = ctx.download(ptrs["dbfs_minmax"], 16, np.float64)
        out["dBfs_min"], out["dBfs_max"] = float(mm[0]), float(mm[1])
        return out
    finally:
        for p in list(ptrs.values()) + [d_in]:
            ctx.free(p)


def _check_case(pkg, ctx, fmt, n, width, samples, ch=False, wf=False, data=None, want_m=None, window="hann", gain=3.0, rng=50.0):
    if data is None:
        data = siggen.generate(fmt, GEN, samples)
    win, weight = pyoracle.window(window, n)
    lut = _lut()
    want = peakref.expected(fmt, data, n, win, 1.0 / weight, gain, rng, lut, width, ch, wf)
    if want_m is not None:
        assert want["M"] == want_m, (want["M"], want_m)
    if want["M"] >= 2:
        # every case has all M sub-frames in all but its last column by construction: nothing else is left out by the existence mask
        assert all(c == want["M"] for c in want["counts"][:-1]), want["counts"]
    assert pkg.binding.peak_subframes(fmt, n, data.size, width) == (want["M"], want["counts"][-1])
    plan = ctx.plan(fmt, n, win, 1.0 / weight, gain, rng, lut, ch, wf, detector="peak")
    try:
        kernels = ["scratch"] + (["frames"] if 64 <= n <= 1024 else [])
        for force in kernels:
            plan.force_kernel(force)
            name = plan.kernel_name(data.size, width)
            if want["M"] >= 2:
                assert name == ("frames_peak" if force == "frames" else "scratch_radix2"), name
            got = _execute(ctx, plan, data, width, n, len(lut))
            peakref.assert_same(got, want, "%s n=%d M=%d %s" % (fmt, n, want["M"], name))
    finally:
        plan.close()
    return want


# (format, n, M, width, extra samples -> fractional stride unless a multiple of width - 1, L/R split, waterfall)
CASES = [
    ("CU8", 32, 2, 70, 0, False, False),
    ("CU8", 64, 2, 70, 0, False, False),
    ("CU8", 256, 3, 45, 17, False, True),
    ("CU8", 512, 7, 37, 5, True, False),
    ("CU8", 1024, 2, 67, 0, False, False),            # a ragged last group
    ("CU8", 1024, 3, 33, 7, False, True),
    ("CS16", 64, 7, 131, 11, True, True),
    ("CS16", 128, 3, 259, 0, False, False),
    ("CS16", 1024, 2, 40, 3, True, False),
    ("CS16", 2048, 3, 9, 4, False, False),
    ("CS12", 256, 2, 50, 0, False, False),
    ("CS12", 512, 3, 35, 9, False, True),
    ("CS12", 8192, 2, 5, 0, True, False),
    ("CF32", 64, 3, 100, 13, False, False),
    ("CF32", 512, 2, 66, 0, True, True),
    ("CF32", 1024, 7, 34, 6, False, False),
    ("CF32", 16384, 2, 3, 0, False, False),
    ("CF64", 256, 7, 21, 2, False, False),
    ("CF64", 1024, 2, 36, 0, True, False),
    ("CF64", 32, 3, 40, 1, False, True),
    ("CU4", 128, 2, 33, 0, False, False),
    ("CS4", 256, 3, 20, 5, False, False),
    ("CS8", 512, 2, 40, 0, False, True),
    ("CU12", 64, 3, 66, 2, False, False),
    ("CU16", 1024, 2, 34, 0, False, False),
    ("CU32", 128, 3, 30, 1, True, False),
    ("CS32", 256, 2, 35, 0, False, False),
    ("CU64", 64, 2, 40, 3, False, False),
    ("CS64", 512, 3, 33, 0, False, True),
]


@pytest.mark.parametrize("fmt,n,M,width,extra,ch,wf", CASES)
def test_peak_reply_matches_the_folded_oracle_planes(pkg, ctx, fmt, n, M, width, extra, ch, wf):
    _check_case(pkg, ctx, fmt, n, width, _samples(n, width, M, extra), ch, wf, want_m=M)


@pytest.mark.parametrize("fmt,n", [("CU8", 64), ("CS16", 32)])
def test_hundreds_of_subframes_per_column(pkg, ctx, fmt, n):
    _check_case(pkg, ctx, fmt, n, 5, _samples(n, 5, 300, 2), want_m=300)


@pytest.mark.parametrize("fmt,n,width", [("CU8", 256, 41), ("CF32", 64, 70), ("CS16", 2048, 6)])
def test_m_flips_from_one_to_two_at_twice_n(pkg, ctx, fmt, n, width):
    """stride just below 2n: the reply is the sample detector's, byte for byte, from the same kernel; at 2n: two sub-frames."""
    win, weight = pyoracle.window("hann", n)
    lut = _lut()
    below = siggen.generate(fmt, GEN, n + (width - 1) * 2 * n - 1)
    assert pkg.binding.peak_subframes(fmt, n, below.size, width)[0] == 1
    replies, names = {}, {}
    for det in ("sample", "peak"):
        plan = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, lut, detector=det)
        names[det] = plan.kernel_name(below.size, width)
        replies[det] = _execute(ctx, plan, below, width, n, len(lut))
        plan.close()
    assert names["peak"] == names["sample"] and names["peak"] in ("frames", "scratch_radix2")
    replies["sample"]["c_hist"] = replies["sample"]["c_hist"].astype(np.int64)
    replies["sample"]["cB_hist"] = replies["sample"]["cB_hist"].astype(np.int64)
    peakref.assert_same(replies["peak"], replies["sample"], "M = 1")
    peakref.assert_same(replies["peak"], pyoracle.render(fmt, below, n, win, 1.0 / weight, 3.0, 50.0, lut, width), "M = 1 vs oracle")
    _check_case(pkg, ctx, fmt, n, width, n + (width - 1) * 2 * n, want_m=2)


def test_nan_and_infinities_in_different_subframes_of_one_column(pkg, ctx):
    n, width, M = 64, 20, 3
    samples = _samples(n, width, M, 0)
    data = siggen.generate("CF32", GEN, samples)
    f = data.view("<f4").reshape(-1, 2)
    stride = M * n
    f[3 * stride + 5, 0] = np.nan                  # column 3, sub-frame 0
    f[3 * stride + n + 9, 1] = np.inf              # column 3, sub-frame 1
    f[3 * stride + 2 * n + 1, 0] = -np.inf         # column 3, sub-frame 2
    for j in range(M):
        f[7 * stride + j * n + 3, 0] = np.nan      # column 7: a NaN in every sub-frame stays a NaN
    f[9 * stride + n + 2, 0] = np.nan              # column 9: a NaN in the middle sub-frame only gives way to numbers
    want = _check_case(pkg, ctx, "CF32", n, width, samples, data=data, want_m=M)
    assert want["gauge_mins"][7] == 255 and want["gauge_maxs"][7] == 0      # all NaN: the column's range keeps its initial (0, -200)


def test_sp_render_named_plan_cache_and_bad_detector(pkg, ctx):
    n, width, M = 256, 60, 3
    fmt = "CS16"
    data = siggen.generate(fmt, GEN, _samples(n, width, M, 7))
    win, weight = pyoracle.window("hann", n)
    lut = _lut()
    args = (fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width)
    want_s = pyoracle.render(*args)
    want_p = peakref.expected(*args)
    before = ctx.plan_creations()
    for det, want in (("sample", want_s), ("peak", want_p), ("sample", want_s), ("peak", want_p), ("peak", want_p)):
        peakref.assert_same(ctx.render(*args, detector=det), want, "sp_render " + det)
    assert ctx.plan_creations() == before + 4          # the detector is part of the plan-cache key; a repeat builds nothing
    assert ctx.last_upload_bytes() == data.size       # a peak request takes the contiguous upload
    peakref.assert_same(ctx.render(*args), want_s, "sample after peak")
    assert ctx.last_upload_bytes() < data.size        # ... and the sample detector's sparse upload is what it was
    # by names
    wn, ck, L = pkg.binding.named_resolve("hann", "viridis")
    lut_v = np.zeros((L, 3), np.uint8)
    import ctypes as C
    n_len = C.c_int32()
    pkg.Library.get().L.sp_cmap(ck.encode(), lut_v.ctypes.data_as(C.c_void_p), L, C.byref(n_len))
    lut_v[0] = 0
    lut_v[-1] = 255
    want_n = peakref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut_v, width)
    peakref.assert_same(ctx.render_named(fmt, data, n, "hann", "viridis", 3.0, 50.0, width, detector="peak"), want_n, "sp_render_named_ex")
    peakref.assert_same(ctx.render_named(fmt, data, n, "hann", "viridis", 3.0, 50.0, width),
                        pyoracle.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut_v, width), "sp_render_named")
    # any other value: an error, never a different image
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, 1.0 / weight, 3.0, 50.0, lut, False, False)
    req.detector = 2
    h = C.c_void_p()
    assert ctx.lib.L.sp_plan_create(ctx.h, C.byref(req), C.byref(h)) == -1
    rep = pkg.binding._Reply()
    assert ctx.lib.L.sp_render(ctx.h, C.byref(req), data.ctypes.data_as(C.c_void_p), data.size, width, C.byref(rep)) == -1
    nr = pkg.binding._NamedRequest(b"cs16", b"hann", b"viridis", n, 0, 0, 3.0, 50.0)
    assert ctx.lib.L.sp_render_named_ex(ctx.h, C.byref(nr), -1, data.ctypes.data_as(C.c_void_p), data.size, width, C.byref(rep)) == -1


def test_chunked_sp_render_and_execute_from_host(pkg, ctx):
    """A request large enough to be pipelined in chunks (>= 16 MiB of samples + image, width >= 1024): every chunk needs the samples up
    to the end of its last column's last sub-frame."""
    fmt, n, width, M = "CU8", 512, 1100, 14
    data = siggen.generate(fmt, GEN, _samples(n, width, M, 333))
    assert data.size + 4 * width * n >= 16 << 20 and width >= 1024      # the documented threshold (spectroplot_hip.h, sp_context_last_upload_bytes)
    win, weight = pyoracle.window("blackmanHarris", n)
    lut = _lut()
    want = peakref.expected(fmt, data, n, win, 1.0 / weight, 6.0, 60.0, lut, width)
    assert want["M"] == M
    got = ctx.render(fmt, data, n, win, 1.0 / weight, 6.0, 60.0, lut, width, detector="peak")
    peakref.assert_same(got, want, "chunked sp_render")
    assert ctx.last_upload_bytes() == data.size
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 60.0, lut, detector="peak")
    try:
        peakref.assert_same(_execute(ctx, plan, data, width, n, len(lut), from_host=True), want, "sp_plan_execute_from_host")
        assert ctx.last_upload_bytes() == data.size
    finally:
        plan.close()


def test_sp_render_strip_honours_the_detector(pkg, ctx):
    """sp_render_strip: the peak strip lands in its band of a wider image, rows image_width pixels apart, the rest untouched."""
    import ctypes as C
    fmt, n, width, image_width, offset = "CS16", 128, 24, 40, 8
    data = siggen.generate(fmt, GEN, _samples(n, width, 3, 5))
    win, weight = pyoracle.window("hann", n)
    lut = _lut()
    want = peakref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width)
    req, keep = pkg.binding._make_request(pkg.parse_format(fmt)[0], n, win, 1.0 / weight, 3.0, 50.0, lut, False, False, "peak")
    image = np.full((n, image_width, 4), 0x5A, np.uint8)
    small = {k: np.zeros(width, np.uint8) for k in ("gauge_mins", "gauge_maxs", "gauge_amps")}
    c_hist, cb_hist, mm = np.zeros(len(lut), np.uint64), np.zeros(1000, np.uint64), np.zeros(2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rep = pkg.binding._Reply(C.c_void_p(image.ctypes.data + 4 * offset), p(small["gauge_mins"]), p(small["gauge_maxs"]), p(small["gauge_amps"]),
                             p(c_hist), p(cb_hist), p(mm))
    ctx._chk(ctx.lib.L.sp_render_strip(ctx.h, C.byref(req), p(data), data.size, width, C.byref(rep), image_width))
    got = dict(small, rgba=np.ascontiguousarray(image[:, offset:offset + width]).ravel(), c_hist=c_hist, cB_hist=cb_hist,
               dBfs_min=float(mm[0]), dBfs_max=float(mm[1]))
    peakref.assert_same(got, want, "sp_render_strip")
    assert (image[:, :offset] == 0x5A).all() and (image[:, offset + width:] == 0x5A).all()


def test_sharding_refuses_a_peak_plan(pkg, ctx):
    from spectroplot_js_amd import sharding
    win, weight = pyoracle.window("hann", 128)
    plan = ctx.plan("CU8", 128, win, 1.0 / weight, 3.0, 50.0, _lut(), detector="peak")
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            sharding.render_sharded_device(plan, None, 64)
        assert e.value.status == -4 and "peak" in str(e.value)
    finally:
        plan.close()


def test_batches_and_groups_refuse_a_peak_plan(pkg, ctx):
    fmt, n, width = "CU8", 128, 20
    data = siggen.generate(fmt, GEN, _samples(n, width, 3, 0))
    win, weight = pyoracle.window("hann", n)
    lut = _lut()
    with pytest.raises(pkg.SpectroplotError) as e:
        ctx.render_batch(fmt, [data, data], n, win, 1.0 / weight, 3.0, 50.0, lut, [width, width], detector="peak")
    assert e.value.status == -4 and "peak" in str(e.value)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, lut, detector="peak")
    try:
        d_in = ctx.alloc(data.size)
        with pytest.raises(pkg.SpectroplotError) as e:
            plan.execute_batch([(d_in, data.size, width, {})])
        assert e.value.status == -4 and "peak" in str(e.value)
        ctx.free(d_in)
    finally:
        plan.close()
    g2 = pkg.Group([0, 0])               # two members: no slice is rendered as "sample" either
    try:
        for gather in ("device", "host"):
            with pytest.raises(pkg.SpectroplotError) as e:
                g2.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width, detector="peak", gather=gather)
            assert e.value.status == -4 and "peak" in str(e.value)
    finally:
        g2.close()
    g = pkg.Group([0])
    try:
        with pytest.raises(pkg.SpectroplotError) as e:
            g.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width, detector="peak")
        assert e.value.status == -4 and "peak" in str(e.value)
        peakref.assert_same(g.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width),
                            pyoracle.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width), "group, sample detector")
    finally:
        g.close()
    # the batch entry points still render a sample request
    outs = ctx.render_batch(fmt, [data], n, win, 1.0 / weight, 3.0, 50.0, lut, [width])
    peakref.assert_same(outs[0], pyoracle.render(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, lut, width), "batch, sample detector")


@pytest.mark.parametrize("n", [256, 2048])
def test_a_burst_between_two_columns_is_in_the_picture(pkg, ctx, n):
    """The point of the detector, without an oracle: a silent CU8 capture with one n-sample tone burst between two reference frames.
    The sample detector shows no pixel above the floor's colour index; the peak detector shows the tone's bin in exactly the column
    that owns the burst."""
    width, M, col, sub, k = 64, 5, 23, 3, n // 8
    samples = _samples(n, width, M, 0)
    stride = M * n
    data = np.full(2 * samples, 128, np.uint8)
    t = np.arange(n)
    start = col * stride + sub * n
    data[2 * start:2 * (start + n):2] = np.round(128 + 100 * np.cos(2 * np.pi * k * t / n)).astype(np.uint8)
    data[2 * start + 1:2 * (start + n):2] = np.round(128 + 100 * np.sin(2 * np.pi * k * t / n)).astype(np.uint8)
    win, weight = pyoracle.window("hann", n)
    L = 256
    lut = np.stack([np.arange(L), np.zeros(L, int), np.zeros(L, int)], axis=1).astype(np.uint8)    # red channel = colour index
    quiet = ctx.render("CU8", data, n, win, 1.0 / weight, 0.0, 60.0, lut, width)
    held = ctx.render("CU8", data, n, win, 1.0 / weight, 0.0, 60.0, lut, width, detector="peak")
    img_q = quiet["rgba"].reshape(n, width, 4)[:, :, 0]
    img_h = held["rgba"].reshape(n, width, 4)[:, :, 0]
    floor = int(img_q.max())
    assert (img_q[:, 0] == img_q[:, col]).all() and floor < 200          # the burst is not in the reference's picture
    y = n // 2 - k                                                       # worker.js:90: row of bin k
    assert int(img_h[y, col]) > floor + 60
    above = np.argwhere(img_h > floor)
    assert len(above) and set(above[:, 1].tolist()) == {col}             # ... and in no other column
    assert held["gauge_maxs"][col] > quiet["gauge_maxs"][col] and held["dBfs_max"] > quiet["dBfs_max"] + 20
