"""The exact lagged covariances as a torch tensor (spectroplot-js_amd/tensor.py): the same bits as Context.render_lagcov and
tests/lagcovref.py on a stream that is not torch's default, the context's stream binding left as it was; and the numpy helper on a
reply - the correlation coefficient normalised by the lag-0 autocovariances."""
import numpy as np
import pytest
import torch

import bandref
import lagcovref
import powerref
from __graft_entry__ import load_package
from test_mean_gpu import _reference

pytestmark = pytest.mark.gpu
FMT, N, WIDTH, LAGS = "CF32", 64, 37, 5
BANDS = [(0, N), (N // 4, N // 2), (N // 2, N // 2 + 1)]
PAIRS = [(0, 0), (1, 1), (2, 2), (1, 2), (2, 1)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def test_tensor_lagcov_is_render_lagcov_on_a_side_stream(pkg, ctx):
    from spectroplot_js_amd import tensor
    data, win, bn, plane, _ = _reference(FMT, N, WIDTH, False, N // 2 + 3)
    want = lagcovref.expected(bandref.expected(plane, BANDS), PAIRS, LAGS)
    rendered = ctx.render_lagcov(FMT, data, N, win, bn, 3.0, 50.0, WIDTH, BANDS, PAIRS, LAGS, fill=0xAB)
    lagcovref.assert_same(rendered, want, "Context.render_lagcov")
    plan = ctx.plan(FMT, N, win, bn, 3.0, 50.0, powerref._LUT)
    try:
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(data.copy()).to(dev)
        before = ctx.get_stream()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(dev) == side
            v = tensor.lagcov(plan, capture, WIDTH, BANDS, PAIRS, LAGS)
            # queued right behind the sums on the same stream, no synchronisation in between
            twice = v[1] + v[1]
            series = tensor.bandpower(plan, capture, WIDTH, BANDS)
            host = [t.cpu().numpy() for t in (v, twice, series)]                       # (the copies synchronise)
        assert ctx.get_stream() == before
        assert v.dtype == torch.float64 and tuple(v.shape) == (3, len(PAIRS), LAGS) and v.device == capture.device and v.is_contiguous()
        lagcovref.assert_same(host[0], want, "tensor.lagcov")
        assert np.array_equal(host[0].view(np.uint64), rendered.view(np.uint64))
        assert np.array_equal(host[1].view(np.uint64), (rendered[1] * 2.0).view(np.uint64))            # (a doubling is exact)
        lagcovref.assert_same(host[0], lagcovref.expected(host[2], PAIRS, LAGS), "tensor.lagcov of tensor.bandpower's series")
        with pytest.raises(pkg.SpectroplotError):
            tensor.lagcov(plan, torch.from_numpy(data.copy()), WIDTH, BANDS, PAIRS, LAGS)              # a host tensor
        assert ctx.get_stream() == before
        zero = tensor.lagcov(plan, capture, LAGS - 2, BANDS, PAIRS, LAGS)                              # fewer frames than lags: N = 0
        assert tuple(zero.shape) == (3, len(PAIRS), LAGS) and not zero.cpu().numpy().view(np.uint64).any()
        none = tensor.lagcov(plan, capture, WIDTH, BANDS, [], LAGS)
        assert tuple(none.shape) == (3, 0, LAGS)
    finally:
        plan.close()
    # the coefficient: 1 at lag 0 of an auto pair, symmetric at lag 0 of a cross pair and its reverse, within [-1, 1] there
    r_auto = pkg.lag_correlation(rendered[1, 1], rendered[1, 1, 0], rendered[1, 1, 0])
    assert r_auto[0] == 1.0 and r_auto.shape == (LAGS,)
    r_ab = pkg.lag_correlation(rendered[1, 3], rendered[1, 1, 0], rendered[1, 2, 0])
    r_ba = pkg.lag_correlation(rendered[1, 4], rendered[1, 2, 0], rendered[1, 1, 0])
    assert r_ab[0] == r_ba[0] and abs(r_ab[0]) <= 1.0
    degenerate = pkg.lag_correlation([0.0, 1.0], 0.0, 1.0)                                             # a series without a variance
    assert np.isnan(degenerate[0]) and np.isinf(degenerate[1])
