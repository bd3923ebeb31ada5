"""The burst measurements as torch tensors (spectroplot-js_amd/tensor.py): tensor.pulses on a stream that is not torch's default one
against Context.render_pulses of the same request and against tests/pulseref.py, bit for bit, with the context's stream binding left
as it was."""
import numpy as np
import pytest
import torch

import powerref
from __graft_entry__ import load_package
from test_pulses_gpu import _oracle_pulses, as_bits, assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def test_tensor_pulses_on_a_side_stream_is_render_pulses(pkg, ctx):
    from spectroplot_js_amd import tensor
    fmt, n, width, m = "CS16", 256, 300, 12
    data, win, bn, bands, hi, lo, want = _oracle_pulses(fmt, n, width, False)
    assert (want[0] > 0).any() and (want[0] > m).any() or (want[4] >= 0).any()
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    try:
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(np.array(data)).to(dev)
        before = ctx.get_stream()
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            reply = tensor.pulses(plan, capture, width, bands, hi, lo, m)
            # torch's arithmetic on the reply, queued behind it on the same stream: the mean level of every listed burst
            listed = reply[4] >= 0
            widths = (reply[1][:, :, 1] - reply[1][:, :, 0]).to(torch.float64)
            mean = torch.where(listed, reply[2] / widths, torch.zeros_like(widths))
            host = [t.cpu().numpy() for t in reply + (mean,)]                                  # (the copies synchronise)
        assert ctx.get_stream() == before
        assert [tuple(t.shape) for t in reply] == [(len(bands),), (len(bands), m, 2), (len(bands), m), (len(bands), m), (len(bands), m)]
        assert [t.dtype for t in reply] == [torch.int32, torch.int32, torch.float64, torch.float64, torch.int32]
        assert all(t.device == capture.device and t.is_contiguous() for t in reply)
        got = as_bits((host[0].view(np.uint32),) + tuple(host[1:5]))
        assert_same(got, want, "tensor.pulses")
        rendered = ctx.render_pulses(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, m)
        assert_same(got, as_bits(rendered), "tensor.pulses against Context.render_pulses")
        with np.errstate(all="ignore"):
            e, w = rendered[2], (rendered[1][:, :, 1] - rendered[1][:, :, 0]).astype(np.float64)
            on = rendered[4] >= 0
            assert np.array_equal(host[5][on], (e / w)[on]) and (host[5][~on] == 0).all()
        with pytest.raises(pkg.SpectroplotError) as err:
            tensor.pulses(plan, capture, width, bands, 1.0, 2.0, m)
        assert err.value.status == -1 and ctx.get_stream() == before
        counts = tensor.pulses(plan, capture, width, bands, hi, lo, 0)                         # counts alone
        assert counts[0].cpu().numpy().view(np.uint32).tolist() == want[0].tolist() and all(t.numel() == 0 for t in counts[1:])
    finally:
        ctx.synchronize()
        plan.close()
