"""The exact spectral moments as a torch tensor (spectroplot-js_amd/tensor.py): the same bits as the ctypes path and tests/momentref.py
on a stream that is not torch's default, the context's stream binding left as it was, and the centroid of a single tone."""
import numpy as np
import pytest
import torch

import bandref
import momentref
import powerref
from __graft_entry__ import load_package
from oracle import pyoracle
from test_mean_gpu import _reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _ctypes_moments(ctx, plan, data, width, bands, order):
    size = 8 * (order + 1) * len(bands) * width
    d_in, d_out = ctx.alloc(data.size), ctx.alloc(size)
    try:
        ctx.upload(d_in, data)
        plan.execute_moments(d_in, data.size, width, bands, order, d_out)
        ctx.synchronize()
        return ctx.download(d_out, size, np.float64).reshape(order + 1, len(bands), width)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


@pytest.mark.parametrize("order", [1, 2])
def test_tensor_moments_is_the_ctypes_path_on_a_side_stream(pkg, ctx, order):
    from spectroplot_js_amd import tensor
    fmt, n, width = "CF32", 64, 37
    data, win, bn, _, _ = _reference(fmt, n, width, False, n // 2 + 3)
    bands = bandref.standard_bands(n)
    want = momentref.expected(_reference(fmt, n, width, False, n // 2 + 3)[3], bands, order)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    try:
        c_got = _ctypes_moments(ctx, plan, data, width, bands, order)
        momentref.assert_same(c_got, want, "ctypes")
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(data.copy()).to(dev)
        before = ctx.get_stream()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(dev) == side
            m = tensor.moments(plan, capture, width, bands) if order == 1 else tensor.moments(plan, capture, width, bands, order=2)
            # queued right behind the moments on the same stream, no synchronisation in between
            row = m[1] / m[0]
            series = tensor.bandpower(plan, capture, width, bands)
            host = [t.cpu().numpy() for t in (m, row, series)]                      # (the copies synchronise)
        assert ctx.get_stream() == before
        assert m.dtype == torch.float64 and tuple(m.shape) == (order + 1, len(bands), width) and m.device == capture.device and m.is_contiguous()
        momentref.assert_same(host[0], want, "tensor.moments")
        assert np.array_equal(host[0].view(np.uint64), c_got.view(np.uint64))
        with np.errstate(all="ignore"):
            assert np.array_equal(host[1], want[1] / want[0], equal_nan=True)
        assert np.array_equal(host[2].view(np.uint64), host[0][0].view(np.uint64))     # m[0] is tensor.bandpower's series
        with pytest.raises(pkg.SpectroplotError) as e:
            tensor.moments(plan, capture, width, bands, order=3)
        assert e.value.status == -1 and ctx.get_stream() == before
        with pytest.raises(pkg.SpectroplotError):
            tensor.moments(plan, torch.from_numpy(data.copy()), width, bands)
        assert tuple(tensor.moments(plan, capture, 0, bands).shape) == (2, len(bands), 0)
    finally:
        plan.close()


def test_centroid_of_a_single_tone(pkg, ctx):
    """A complex exponential between two bins: the centroid of a band around it lands within half a bin of the tone, where the peak
    track could only name a bin."""
    from spectroplot_js_amd import tensor
    n, width, stride, f = 256, 24, 100, 0.1337
    t = np.arange(n + (width - 1) * stride, dtype=np.float64)
    iq = np.empty((t.size, 2), np.float32)
    iq[:, 0], iq[:, 1] = 0.5 * np.cos(2 * np.pi * f * t), 0.5 * np.sin(2 * np.pi * f * t)
    data = iq.reshape(-1).view(np.uint8).copy()
    win, weight = pyoracle.window("hann", n)
    bands = [pkg.band_rows(n, f - 0.05, f + 0.05), pkg.band_rows(n, -0.5, 0.5)]
    assert bands[1] == (0, n) and 20 <= bands[0][1] - bands[0][0] <= 27
    plan = ctx.plan("CF32", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    try:
        dev = torch.device("cuda", 0)
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            m = tensor.moments(plan, torch.from_numpy(data).to(dev), width, bands).cpu().numpy()
    finally:
        plan.close()
    freq = pkg.centroid_freq(n, bands, m[0], m[1])
    assert freq.shape == (2, width) and np.isfinite(freq).all()
    assert (np.abs(freq[0] - f) < 0.5 / n).all(), np.abs(freq[0] - f).max() * n
    # the same from the plane on the host: the centroid row is y0 + m1 / m0
    y0 = bands[0][0]
    rows = y0 + m[1, 0] / m[0, 0]
    assert (np.abs((n / 2 - rows) / n - freq[0]) < 1e-12).all()
