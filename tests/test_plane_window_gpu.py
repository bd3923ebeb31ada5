"""Host-fed plane consumers (sp_render_mean, sp_render_bandpower, sp_render_track) whose chunks and window blocks do not line up: the
streamer cuts a request on multiples of 32 frames, and a window of five frames cuts every chunk into blocks that end elsewhere.  The
reply must be what tests/meanref.py, bandref.py and trackref.py make of the oracle's plane - the chunked tests' own comparisons - and,
bit for bit, what the default window gives.

The request is the chunked tests' (test_mean_gpu.py, test_band_gpu.py, test_track_gpu.py): its capture and plane are computed once for
all of them."""
import numpy as np
import pytest

import bandref
import meanref
import trackref
from __graft_entry__ import load_package
from test_band_gpu import _want as band_series
from test_mean_gpu import GARBAGE, _reference

pytestmark = pytest.mark.gpu

FMT, N, WIDTH = "CF32", 1024, 2048      # stride n, 16 MiB: the smallest request the streamer cuts
BLOCK_FRAMES = 5                        # does not divide the chunks' 32


@pytest.fixture(scope="module")
def ctx():
    c = load_package().Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _mean(ctx, data, win, bn, plane, mean):
    return (lambda: ctx.render_mean(FMT, data, N, win, bn, 3.0, 50.0, WIDTH, fill=GARBAGE),
            lambda got, what: meanref.assert_same(got, mean, what),
            _same_bits)


def _bandpower(ctx, data, win, bn, plane, mean):
    bands = bandref.standard_bands(N)
    want = band_series(FMT, N, WIDTH, False, N)       # (bandref.expected of the plane and these bands, shared with test_band_gpu.py)
    return (lambda: ctx.render_bandpower(FMT, data, N, win, bn, 3.0, 50.0, WIDTH, bands, fill=GARBAGE),
            lambda got, what: bandref.assert_same(got, want, what),
            _same_bits)


def _track(ctx, data, win, bn, plane, mean):
    bands = bandref.standard_bands(N)
    want = trackref.expected(plane, bands)
    return (lambda: ctx.render_track(FMT, data, N, win, bn, 3.0, 50.0, WIDTH, bands, fill=GARBAGE),
            lambda got, what: trackref.assert_same(got, want, what),
            lambda a, b: a[0].dtype == np.int32 and np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1]))


@pytest.mark.parametrize("kind", [_mean, _bandpower, _track], ids=["mean", "bandpower", "track"])
def test_window_blocks_that_straddle_the_chunks(ctx, kind):
    data, win, bn, plane, mean = _reference(FMT, N, WIDTH, False, N)
    assert data.size >= 16 << 20
    render, assert_expected, same = kind(ctx, data, win, bn, plane, mean)
    try:
        ctx.set_mean_window(BLOCK_FRAMES * 8 * N)
        got = render()
        assert ctx.last_chunks() > 1
    finally:
        ctx.set_mean_window(0)
    assert_expected(got, "a window of %d frames" % BLOCK_FRAMES)
    default = render()
    assert ctx.last_chunks() > 1
    assert same(got, default), "the window changed the reply"
