"""The occupancy counts as two torch tensors (spectroplot-js_amd/tensor.py): the words of tests/occref.py and of the ctypes path, on the
hopping capture of tests/test_track_gpu.py, ordered on torch's current stream so that what is queued right behind them needs no
synchronisation, and the context's stream binding left as it was."""
import numpy as np
import pytest
import torch

import bandref
import meanref
import occref
import powerref
from __graft_entry__ import load_package
from oracle import pyoracle
from test_track_gpu import hopping

pytestmark = pytest.mark.gpu

CASES = [("CU8", 256, 40, False), ("CF32", 1024, 64, True)]
K_ROTATION = (0.5, 1.0, 2.0, 0.0, 4.0, 1e6, 0.25)      # per row, as in tests/test_occupancy_gpu.py


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _ctypes_occupancy(ctx, plan, data, width, thr, bands):
    count, n = len(bands), plan.n
    d_in, d_t, d_r, d_f = ctx.alloc(data.size), ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(max(4 * count * width, 16))
    try:
        ctx.upload(d_in, data)
        ctx.upload(d_t, np.ascontiguousarray(thr).view(np.uint8))
        plan.execute_occupancy(d_in, data.size, width, d_t, bands, d_r, d_f)
        ctx.synchronize()
        return ctx.download(d_r, 4 * n, np.uint32), ctx.download(d_f, 4 * count * width, np.uint32).reshape(count, width)
    finally:
        for p in (d_in, d_t, d_r, d_f):
            ctx.free(p)


def _as_words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("fmt,n,width,ch", CASES)
@pytest.mark.parametrize("own_stream", [False, True])
def test_tensor_occupancy_is_the_reference_and_orders_what_follows(pkg, ctx, fmt, n, width, ch, own_stream):
    from spectroplot_js_amd import tensor
    data = hopping(fmt, n + (width - 1) * (n // 2 + 3))
    win, weight = pyoracle.window("hann", n)
    want_plane = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, ch)["power"]
    powerref.assert_telling(want_plane[:, 1:] if ch else want_plane)
    bands = bandref.standard_bands(n) + [pkg.band_rows(n, -0.125, 0.25)]
    thr = np.array([K_ROTATION[y % len(K_ROTATION)] for y in range(n)]) * meanref.expected(want_plane)
    want = occref.expected(want_plane, thr, bands)
    share = int(want[0].astype(np.int64).sum()) / float(n * width)
    assert 0.02 <= share <= 0.98 and len(np.unique(want[1][2])) >= 8 and (want[0] == 0).any() and (want[0] == width).any()
    level = float(np.median(want_plane))
    want_level = occref.expected(want_plane, np.full(n, level), bands)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, ch)
    try:
        occref.assert_same(_ctypes_occupancy(ctx, plan, data, width, thr, bands), want, "ctypes")
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(data).to(dev)
        d_thr = torch.from_numpy(thr).to(dev)
        before = ctx.get_stream()
        stream = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            rows, frames = tensor.occupancy(plan, capture, width, d_thr, bands)
            # queued right behind the counts on the same stream, no synchronisation in between
            hits = rows.to(torch.int64).cumsum(0)          # (integers: torch's division by a number is no IEEE division on the device)
            busiest = frames[2].argmax()
            r2, f2 = tensor.occupancy(plan, capture, width, level, bands)          # a Python float: every row's threshold
            plane = tensor.power(plan, capture, width)
            host = [t.cpu().numpy() for t in (hits, busiest, plane)]                # (the copies synchronise)
        assert ctx.get_stream() == before
        assert rows.dtype == torch.int32 and frames.dtype == torch.int32 and rows.device == frames.device == capture.device
        assert tuple(rows.shape) == (n,) and tuple(frames.shape) == (len(bands), width) and rows.is_contiguous() and frames.is_contiguous()
        occref.assert_same((_as_words(rows), _as_words(frames)), want, "tensor.occupancy")
        occref.assert_same((_as_words(r2), _as_words(f2)), want_level, "tensor.occupancy with a float")
        assert np.array_equal(host[0], np.cumsum(want[0].astype(np.int64)))
        assert int(host[1]) == int(np.argmax(want[1][2]))
        powerref.assert_same(host[2], want_plane, "tensor.power behind tensor.occupancy")
        # the context still computes on its own binding afterwards
        occref.assert_same(_ctypes_occupancy(ctx, plan, data, width, thr, bands), want, "ctypes afterwards")
    finally:
        plan.close()


def test_tensor_occupancy_restores_a_bound_stream_and_refuses_what_the_library_refuses(pkg, ctx):
    from spectroplot_js_amd import tensor
    n, width = 128, 50
    data = hopping("CS16", n + (width - 1) * 77)
    win, weight = pyoracle.window("hann", n)
    plan = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    dev = torch.device("cuda", 0)
    bound = torch.cuda.Stream(device=dev)
    ctx.set_stream(bound.cuda_stream)
    bands = [(0, n), (17, 18), (40, 40)]
    plane = powerref.expected("CS16", data, n, win, 1.0 / weight, 3.0, 50.0, width)["power"]
    level = float(np.median(plane))
    try:
        other = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(other):
            got = tuple(_as_words(t) for t in tensor.occupancy(plan, torch.from_numpy(data).to(dev), width, level, bands))
        assert ctx.get_stream() == bound.cuda_stream
        want = occref.expected(plane, np.full(n, level), bands)
        assert 0.02 * n * width <= int(want[0].sum()) <= 0.98 * n * width
        occref.assert_same(got, want, "on another stream than the bound one")
        assert np.array_equal(got[1][1], (plane[:, 17] >= level).astype(np.uint32)) and not got[1][2].any()
        capture = torch.from_numpy(data).to(dev)
        with pytest.raises(pkg.SpectroplotError):
            tensor.occupancy(plan, torch.from_numpy(data), width, level, bands)
        for bad in ([(0, n + 1)], [(3, 2)], [(0, 1)] * 65):
            with pytest.raises(pkg.SpectroplotError) as e:
                tensor.occupancy(plan, capture, width, level, bad)
            assert e.value.status == -1
        for bad in (torch.zeros(n - 1, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
                    torch.zeros(n, dtype=torch.float64), torch.zeros(2 * n, dtype=torch.float64, device=dev)[::2]):
            with pytest.raises(pkg.SpectroplotError) as e:
                tensor.occupancy(plan, capture, width, bad, bands)
            assert e.value.status == -1
        peak_plan = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, detector="peak")
        try:
            with pytest.raises(pkg.SpectroplotError) as e:
                tensor.occupancy(peak_plan, capture, width, level, bands)
            assert e.value.status == -4
        finally:
            peak_plan.close()
        assert ctx.get_stream() == bound.cuda_stream
        rows, frames = tensor.occupancy(plan, capture, 0, level, bands)
        assert tuple(rows.shape) == (n,) and tuple(frames.shape) == (3, 0) and not rows.cpu().numpy().any()      # no frames: n zeros
        rows, frames = tensor.occupancy(plan, capture, width, level)
        assert tuple(frames.shape) == (0, width) and np.array_equal(_as_words(rows), want[0])                     # the rows need no bands
    finally:
        ctx.synchronize()
        ctx.set_stream(0)
        plan.close()
