"""The exact mean-power trace as a torch tensor (spectroplot-js_amd/tensor.py): the same bits as the ctypes path, ordered on torch's
current stream so that what is queued right behind it needs no synchronisation, and the context's stream binding left as it was."""
import numpy as np
import pytest
import torch

import meanref
import powerref
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 1618, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
CASES = [("CS16", 256, 333, False), ("CF32", 1024, 70, True), ("CU8", 2048, 21, False)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _ctypes_mean(ctx, plan, data, width, n):
    d_in, d_m = ctx.alloc(data.size), ctx.alloc(8 * n)
    try:
        ctx.upload(d_in, data)
        plan.execute_mean(d_in, data.size, width, d_m)
        ctx.synchronize()
        return ctx.download(d_m, 8 * n, np.float64)
    finally:
        ctx.free(d_in)
        ctx.free(d_m)


@pytest.mark.parametrize("fmt,n,width,ch", CASES)
@pytest.mark.parametrize("own_stream", [False, True])
def test_tensor_mean_is_the_ctypes_mean_and_orders_what_follows(pkg, ctx, fmt, n, width, ch, own_stream):
    from spectroplot_js_amd import tensor
    data = siggen.generate(fmt, GEN, n + (width - 1) * (n // 2 + 3))
    win, weight = pyoracle.window("hann", n)
    want_plane = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, ch)["power"]
    powerref.assert_telling(want_plane[:, 1:] if ch else want_plane)
    want = meanref.expected(want_plane)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, ch)
    try:
        c_mean = _ctypes_mean(ctx, plan, data, width, n)
        meanref.assert_same(c_mean, want, "ctypes")
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(data).to(dev)
        before = ctx.get_stream()
        stream = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            mean = tensor.mean(plan, capture, width)
            # queued right behind the mean on the same stream, no synchronisation in between
            top = mean.amax()
            doubled = mean * 2.0
            plane = tensor.power(plan, capture, width)
            host = [t.cpu().numpy() for t in (mean, top, doubled, plane)]          # (the copies synchronise)
        assert ctx.get_stream() == before
        assert mean.dtype == torch.float64 and tuple(mean.shape) == (n,) and mean.device == capture.device
        meanref.assert_same(host[0], c_mean, "tensor.mean")
        assert host[1] == c_mean.max() and np.array_equal(host[2], c_mean * 2.0)
        powerref.assert_same(host[3], want_plane, "tensor.power behind tensor.mean")
        # the context still computes on its own binding afterwards
        meanref.assert_same(_ctypes_mean(ctx, plan, data, width, n), c_mean, "ctypes afterwards")
    finally:
        plan.close()


def test_tensor_mean_restores_a_bound_stream_and_refuses_host_tensors(pkg, ctx):
    from spectroplot_js_amd import tensor
    n, width = 128, 50
    data = siggen.generate("CS16", GEN, n + (width - 1) * 77)
    win, weight = pyoracle.window("hann", n)
    plan = ctx.plan("CS16", n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT)
    dev = torch.device("cuda", 0)
    bound = torch.cuda.Stream(device=dev)
    ctx.set_stream(bound.cuda_stream)
    try:
        other = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(other):
            got = tensor.mean(plan, torch.from_numpy(data).to(dev), width).cpu().numpy()
        assert ctx.get_stream() == bound.cuda_stream
        want = meanref.expected(powerref.expected("CS16", data, n, win, 1.0 / weight, 3.0, 50.0, width)["power"])
        meanref.assert_same(got, want, "on another stream than the bound one")
        with pytest.raises(pkg.SpectroplotError):
            tensor.mean(plan, torch.from_numpy(data), width)
        assert ctx.get_stream() == bound.cuda_stream
        empty = tensor.mean(plan, torch.from_numpy(data).to(dev), 0)
        assert tuple(empty.shape) == (n,) and bool(torch.isnan(empty).all())
    finally:
        ctx.synchronize()
        ctx.set_stream(0)
        plan.close()
