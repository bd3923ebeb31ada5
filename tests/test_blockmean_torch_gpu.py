"""The averaged spectrogram and the colouring of a plane as torch tensors (spectroplot-js_amd/tensor.py): on torch's current stream and
on a side stream they are, bit for bit, what the ctypes path replies and what tests/blockmeanref.py makes of the oracle's plane, and the
context's stream binding is left as it was."""
import numpy as np
import pytest
import torch

import blockmeanref
import edgeref
from __graft_entry__ import load_package
from test_mean_gpu import _Out, _reference, _upload

pytestmark = pytest.mark.gpu

CASES = [("CS16", 256, 300, 7, False), ("CF32", 1024, 37, 5, True)]


@pytest.fixture(scope="module")
def ctx():
    c = load_package().Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt,n,width,group,waterfall", CASES)
@pytest.mark.parametrize("own_stream", [False, True])
def test_tensor_blockmean_and_power_to_index_are_the_ctypes_path(ctx, fmt, n, width, group, waterfall, own_stream):
    from spectroplot_js_amd import tensor
    data, win, bn, plane, _ = _reference(fmt, n, width, False, n // 2 + 3)
    want = blockmeanref.expected(plane, group)
    cols = want.shape[0]
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, edgeref.lut(256), False, waterfall)
    d_in = _upload(ctx, data)
    means, image = _Out(ctx, cols * n), _Out(ctx, (cols * n + 7) // 8)
    try:
        plan.execute_blockmean(d_in, data.size, width, group, means.ptr)
        plan.power_to_index(means.ptr, cols, image.ptr)
        ctx.synchronize()
        c_means = means.read("ctypes").reshape(cols, n)
        c_image = image.read("ctypes").view(np.uint8)[:cols * n]
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(np.array(data)).to(dev)
        before = ctx.get_stream()
        stream = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            t_means = tensor.blockmean(plan, capture, width, group)
            t_image = tensor.power_to_index(plan, t_means)          # queued right behind the means, no synchronisation in between
            host = [t.cpu().numpy() for t in (t_means, t_image)]     # (the copies synchronise)
        assert ctx.get_stream() == before
        assert t_means.dtype == torch.float64 and tuple(t_means.shape) == (cols, n) and t_means.device == capture.device
        assert t_image.dtype == torch.uint8 and tuple(t_image.shape) == ((cols, n) if waterfall else (n, cols))
        blockmeanref.assert_same(host[0], want, "tensor.blockmean")
        blockmeanref.assert_same(host[0], c_means, "tensor.blockmean against the ctypes path")
        assert np.array_equal(host[1].reshape(-1), c_image)
        assert len(np.unique(c_image)) > 1
        assert tuple(tensor.blockmean(plan, capture, 0, group).shape) == (0, n)
    finally:
        means.free()
        image.free()
        ctx.free(d_in)
        plan.close()
