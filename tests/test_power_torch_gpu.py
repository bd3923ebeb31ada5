"""The power plane as a torch tensor (spectroplot-js_amd/tensor.py): the same bits as the ctypes path, ordered on torch's current stream
so that a reduction queued right behind it needs no synchronisation, and the context's stream binding left as it was."""
import numpy as np
import pytest
import torch

import powerref
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 1414, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
CASES = [("CS16", 256, 333, False), ("CF32", 1024, 70, True), ("CU8", 2048, 21, False)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _ctypes_planes(ctx, plan, data, width, n):
    d_in, d_p = ctx.alloc(data.size), ctx.alloc(8 * width * n)
    try:
        ctx.upload(d_in, data)
        plan.execute_power(d_in, data.size, width, d_p)
        ctx.synchronize()
        power = ctx.download(d_p, 8 * width * n, np.float64).reshape(width, n)
        plan.power_to_db(d_p, width * n, d_p)
        ctx.synchronize()
        return power, ctx.download(d_p, 8 * width * n, np.float64).reshape(width, n)
    finally:
        ctx.free(d_in)
        ctx.free(d_p)


@pytest.mark.parametrize("fmt,n,width,ch", CASES)
@pytest.mark.parametrize("own_stream", [False, True])
def test_tensor_power_is_the_ctypes_plane_and_orders_what_follows(pkg, ctx, fmt, n, width, ch, own_stream):
    from spectroplot_js_amd import tensor
    data = siggen.generate(fmt, GEN, n + (width - 1) * (n // 2 + 3))
    win, weight = pyoracle.window("hann", n)
    want = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 50.0, width, ch)
    powerref.assert_telling(want["power"][:, 1:] if ch else want["power"])
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 3.0, 50.0, powerref._LUT, ch)
    try:
        c_power, c_db = _ctypes_planes(ctx, plan, data, width, n)
        powerref.assert_same(c_power, want["power"], "ctypes")
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(data).to(dev)
        before = ctx.get_stream()
        stream = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            plane = tensor.power(plan, capture, width)
            # queued right behind the plane on the same stream, no synchronisation in between
            col_max = plane.amax(dim=0)
            row_min = plane[:, 1:].amin(dim=1)
            db = tensor.power(plan, capture, width, db=True)
            filled = torch.full((width, n), -1.0, dtype=torch.float64, device=dev)
            again = tensor.power(plan, capture, width, out=filled)
            host = [t.cpu().numpy() for t in (plane, col_max, row_min, db, again)]          # (the copies synchronise)
        assert ctx.get_stream() == before
        assert plane.dtype == torch.float64 and tuple(plane.shape) == (width, n) and plane.device == capture.device
        assert again.data_ptr() == filled.data_ptr()
        powerref.assert_same(host[0], c_power, "tensor.power")
        powerref.assert_same(host[3], c_db, "tensor.power db")
        powerref.assert_same(host[4], c_power, "tensor.power out=")
        assert np.array_equal(host[1], c_power.max(axis=0)) and np.array_equal(host[2], c_power[:, 1:].min(axis=1))
        # the context still renders on its own binding afterwards
        powerref.assert_same(_ctypes_planes(ctx, plan, data, width, n)[0], c_power, "ctypes afterwards")
    finally:
        plan.close()


def test_tensor_power_restores_a_bound_stream_and_refuses_host_tensors(pkg, ctx):
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
            plane = tensor.power(plan, torch.from_numpy(data).to(dev), width)
            got = plane.cpu().numpy()
        assert ctx.get_stream() == bound.cuda_stream
        want = powerref.expected("CS16", data, n, win, 1.0 / weight, 3.0, 50.0, width)
        powerref.assert_same(got, want["power"], "on another stream than the bound one")
        with pytest.raises(pkg.SpectroplotError):
            tensor.power(plan, torch.from_numpy(data), width)
        with pytest.raises(pkg.SpectroplotError):
            tensor.power(plan, torch.from_numpy(data).to(dev), width, out=torch.empty(3, dtype=torch.float64, device=dev))
        assert ctx.get_stream() == bound.cuda_stream
        empty = tensor.power(plan, torch.from_numpy(data).to(dev), 0)
        assert tuple(empty.shape) == (0, n)
    finally:
        ctx.synchronize()
        ctx.set_stream(0)
        plan.close()
