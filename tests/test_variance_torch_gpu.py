"""The exact variance sums as a torch tensor (spectroplot-js_amd/tensor.py): the same bits as the ctypes path and tests/varianceref.py on
a stream that is not torch's default, the context's stream binding left as it was; and the two numpy helpers on a reply - the variance
and the spectral kurtosis - against rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import powerref
import varianceref
from __graft_entry__ import load_package
from test_mean_gpu import _reference

pytestmark = pytest.mark.gpu
FMT, N, WIDTH = "CF32", 64, 37


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _ctypes_variance(ctx, plan, data, width, n):
    d_in, d_out = ctx.alloc(data.size), ctx.alloc(24 * n)
    try:
        ctx.upload(d_in, data)
        plan.execute_variance(d_in, data.size, width, d_out)
        ctx.synchronize()
        return ctx.download(d_out, 24 * n, np.float64).reshape(3, n)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


@pytest.fixture(scope="module")
def reply(ctx):
    """(the reply of Plan.execute_variance, the reference) for the request the tests share."""
    data, win, bn, plane, _ = _reference(FMT, N, WIDTH, False, N // 2 + 3)
    want = varianceref.expected(plane)
    plan = ctx.plan(FMT, N, win, bn, 3.0, 50.0, powerref._LUT)
    try:
        got = _ctypes_variance(ctx, plan, data, WIDTH, N)
    finally:
        plan.close()
    varianceref.assert_same(got, want, "ctypes")
    return got, want


def test_tensor_variance_is_the_ctypes_path_on_a_side_stream(pkg, ctx, reply):
    from spectroplot_js_amd import tensor
    data, win, bn, _, _ = _reference(FMT, N, WIDTH, False, N // 2 + 3)
    c_got, want = reply
    plan = ctx.plan(FMT, N, win, bn, 3.0, 50.0, powerref._LUT)
    try:
        dev = torch.device("cuda", 0)
        capture = torch.from_numpy(data.copy()).to(dev)
        before = ctx.get_stream()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(dev) == side
            v = tensor.variance(plan, capture, WIDTH)
            # queued right behind the sums on the same stream, no synchronisation in between
            twice = v[2] + v[2]
            mean = tensor.mean(plan, capture, WIDTH)
            host = [t.cpu().numpy() for t in (v, twice, mean)]                         # (the copies synchronise)
        assert ctx.get_stream() == before
        assert v.dtype == torch.float64 and tuple(v.shape) == (3, N) and v.device == capture.device and v.is_contiguous()
        varianceref.assert_same(host[0], want, "tensor.variance")
        assert np.array_equal(host[0].view(np.uint64), c_got.view(np.uint64))
        assert np.array_equal(host[1].view(np.uint64), (c_got[2] * 2.0).view(np.uint64))               # (a doubling is exact)
        assert np.array_equal((host[0][0] / np.float64(WIDTH)).view(np.uint64), host[2].view(np.uint64))   # out[0] / W is tensor.mean
        with pytest.raises(pkg.SpectroplotError):
            tensor.variance(plan, torch.from_numpy(data.copy()), WIDTH)               # a host tensor
        assert ctx.get_stream() == before
        zero = tensor.variance(plan, capture, 0)
        assert tuple(zero.shape) == (3, N) and not zero.cpu().numpy().view(np.uint64).any()
    finally:
        plan.close()


def _ulps(got, want):
    """|got - want| in units of the spacing of doubles at `want` (a Fraction), exactly."""
    want_f = float(want)
    return abs(Fraction(float(got)) - want) / Fraction(float(np.spacing(abs(want_f))))


def test_the_helpers_against_rational_arithmetic(pkg, reply):
    """variance_of is one division by an exactly representable integer: at most half an ulp from the quotient of the reply's values, held
    to 1.  spectral_kurtosis performs four roundings - the quotient (W + 1) / (W - 1), its product with sums[2], the square of sums[0]
    and the last division - each at most half an ulp relative: held to 4 ulps, one per operation."""
    got, _ = reply
    w = WIDTH
    for ddof in (0, 1):
        var = pkg.variance_of(got, w, ddof)
        assert var.shape == (N,)
        for y in range(N):
            assert _ulps(var[y], Fraction(float(got[2, y])) / (w * (w - ddof))) <= 1, (ddof, y)
    sk = pkg.spectral_kurtosis(got, w)
    assert sk.shape == (N,) and np.isfinite(sk).all() and (sk >= 0).all() and sk.any()
    for y in range(N):
        exact = Fraction(w + 1, w - 1) * Fraction(float(got[2, y])) / Fraction(float(got[0, y])) ** 2
        assert _ulps(sk[y], exact) <= 4, y
    # what the forms are for: a constant row has variance and kurtosis 0 exactly, a row of no power and a request of no frames give NaN
    flat = np.array([[37.0 * 0.1, 0.0], [37.0 * 0.01, 0.0], [0.0, 0.0]])
    assert pkg.variance_of(flat, 37)[0] == 0.0 and pkg.spectral_kurtosis(flat, 37)[0] == 0.0
    assert np.isnan(pkg.spectral_kurtosis(flat, 37)[1]) and np.isnan(pkg.variance_of(np.zeros((3, 2)), 0)).all()
    assert np.isnan(pkg.variance_of(flat, 1, ddof=1)).all()                          # 0 / 0: one frame has no sample variance
