"""The burst lists as torch tensors (spectroplot-js_amd/tensor.py): the words of tests/burstref.py on bandref's exact sums of the oracle's
plane of tests/test_track_gpu.py's hopping captures, on torch's current stream and on a side stream, chained behind tensor.bandpower
without a host synchronisation, and the context's stream binding left as it was."""
import numpy as np
import pytest
import torch

import bandref
import powerref
from __graft_entry__ import load_package
from test_bursts_gpu import _oracle_reference, assert_same
from test_track_gpu import _hop_reference

pytestmark = pytest.mark.gpu

CASES = [("CS16", 256, 300, False), ("CF32", 1024, 37, True)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _words(pair):
    counts, edges = (t.cpu().numpy() for t in pair)
    assert counts.dtype == np.int32 and edges.dtype == np.int32
    return counts.view(np.uint32), edges


@pytest.mark.parametrize("fmt,n,width,ch", CASES)
@pytest.mark.parametrize("own_stream", [False, True])
def test_tensor_bursts_is_the_reference_and_chains_behind_bandpower(pkg, ctx, fmt, n, width, ch, own_stream):
    from spectroplot_js_amd import tensor
    data, win, bn, bands, hi, lo, want = _oracle_reference(fmt, n, width, ch)
    plane = _hop_reference(fmt, n, width, ch, n // 2 + 3)[3]
    sums = bandref.expected(plane, bands)
    assert (want[0] > 0).any()
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, ch)
    try:
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(np.array(data)).to(dev)
        before = ctx.get_stream()
        stream = torch.cuda.Stream(device=dev) if own_stream else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            series = tensor.bandpower(plan, capture, width, bands)
            # queued right behind the series on the same stream, no synchronisation in between: the library's own scan of it ...
            counts = torch.empty((len(bands),), dtype=torch.int32, device=dev)
            edges = torch.empty((len(bands), 12, 2), dtype=torch.int32, device=dev)
            with tensor._on_current_stream(ctx, dev, (series, counts, edges)):
                ctx.series_bursts(series.data_ptr(), len(bands), width, hi, lo, 12, counts.data_ptr(), edges.data_ptr())
            # ... the one call, and torch's arithmetic on its reply
            direct = tensor.bursts(plan, capture, width, bands, hi, lo, 12)
            listed = (direct[1][:, :, 0] >= 0).sum(dim=1)
            host = [t.cpu().numpy() for t in (series, listed)]                              # (the copies synchronise)
        assert ctx.get_stream() == before
        assert direct[0].device == capture.device and tuple(direct[0].shape) == (len(bands),) and tuple(direct[1].shape) == (len(bands), 12, 2)
        assert direct[1].is_contiguous()
        bandref.assert_same(host[0], sums, "tensor.bandpower")
        assert_same(_words(direct), want, "tensor.bursts")
        assert_same(_words((counts, edges)), want, "series_bursts behind tensor.bandpower")
        assert host[1].tolist() == np.minimum(want[0], 12).tolist()
        # the context still computes on its own binding afterwards
        assert_same(ctx.render_bursts(fmt, data, n, win, bn, 3.0, 50.0, width, bands, hi, lo, 12, channel_mode=ch), want, "ctypes afterwards")
    finally:
        plan.close()


def test_tensor_bursts_restores_a_bound_stream_and_refuses_what_the_library_refuses(pkg, ctx):
    from spectroplot_js_amd import tensor
    fmt, n, width = "CS16", 256, 300
    data, win, bn, bands, hi, lo, want = _oracle_reference(fmt, n, width, False)
    plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT)
    dev = torch.device("cuda", 0)
    bound = torch.cuda.Stream(device=dev)
    ctx.set_stream(bound.cuda_stream)
    try:
        other = torch.cuda.Stream(device=dev)
        capture = torch.from_numpy(np.array(data)).to(dev)
        with torch.cuda.stream(other):
            got = _words(tensor.bursts(plan, capture, width, bands, hi, lo, 12))
        assert ctx.get_stream() == bound.cuda_stream
        assert_same(got, want, "on another stream than the bound one")
        with pytest.raises(pkg.SpectroplotError):
            tensor.bursts(plan, torch.from_numpy(np.array(data)), width, bands, hi, lo, 12)
        for h, l, m in ((float("nan"), 1.0, 4), (1.0, 2.0, 4), (2.0, 1.0, -1), (hi[:3], lo, 4)):
            with pytest.raises(pkg.SpectroplotError) as e:
                tensor.bursts(plan, capture, width, bands, h, l, m)
            assert e.value.status == -1
        peak_plan = ctx.plan(fmt, n, win, bn, 3.0, 50.0, powerref._LUT, detector="peak")
        try:
            with pytest.raises(pkg.SpectroplotError) as e:
                tensor.bursts(peak_plan, capture, width, bands, hi, lo, 4)
            assert e.value.status == -4
        finally:
            peak_plan.close()
        assert ctx.get_stream() == bound.cuda_stream
        counts, edges = _words(tensor.bursts(plan, capture, 0, bands, hi, lo, 3))             # no frames: no bursts
        assert (counts == 0).all() and edges.shape == (len(bands), 3, 2) and (edges == -1).all()
        counts, edges = _words(tensor.bursts(plan, capture, width, bands, hi, lo, 0))         # counts alone
        assert counts.tolist() == want[0].tolist() and edges.size == 0
    finally:
        ctx.synchronize()
        ctx.set_stream(0)
        plan.close()
