"""Expected band-power series (include/spectroplot_hip.h, sp_plan_execute_bandpower): meanref.exact_sum - math.fsum with the NaN, inf
and overflow rules of the header - over a range of image rows of every frame of a power plane, and the rows of a frequency range
(sp_band_rows) restated with math.ceil / math.floor.  Test infrastructure, not a test."""
import math

import numpy as np

import meanref

SP_MAX_BANDS = 64


def expected(plane, bands):
    """f64 [count, width]: out[b, x] = exact_sum(plane[x, y0_b:y1_b]) for a plane f64 [width, n]; an empty band gives +0.0."""
    plane = np.ascontiguousarray(plane, np.float64)
    width = plane.shape[0]
    out = np.zeros((len(bands), width), np.float64)
    for b, (y0, y1) in enumerate(bands):
        for x in range(width):
            out[b, x] = meanref.exact_sum(plane[x, y0:y1])
    return out


def assert_same(got, want, what=""):
    """meanref.same's comparison - the same shape, NaN at the same places (a NaN is any NaN), the same bits everywhere else - of two
    series arrays [count, width], with the first difference in words."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    if meanref.same(got, want):
        return
    na, nb = np.isnan(got), np.isnan(want)
    bad = np.argwhere((na != nb) | (~na & ~nb & (meanref.bits(got) != meanref.bits(want))))
    at = tuple(bad[0])
    raise AssertionError("%s: the series differ in %d of %d values, first at (band, frame) %r: got %r, want %r"
                         % (what, len(bad), want.size, at, got[at], want[at]))


def _clamp(v, n):
    return 0 if v < 0 else n if v > n else int(v)


def band_rows(n, f_lo, f_hi):
    """(y0, y1) of sp_band_rows for a power of two n >= 2 and f_lo <= f_hi, neither a NaN: the rows whose centre frequency
    f(y) = (n/2 - y) / n lies in [f_lo, f_hi].  y0 = clamp(ceil(n/2 - f_hi * n), 0, n), y1 = clamp(floor(n/2 - f_lo * n) + 1, 0, n)
    raised to y0, in f64 in that order (an infinity clamps)."""
    a = float(n // 2) - float(f_hi) * float(n)
    b = float(n // 2) - float(f_lo) * float(n)
    y0 = _clamp(a if math.isinf(a) else math.ceil(a), n)
    y1 = _clamp(b if math.isinf(b) else math.floor(b) + 1, n)
    return y0, max(y0, y1)


def synthetic_plane(seed, n, width):
    """A plane f64 [width, n] for sp_power_bands: meanref's synthetic plane turned, so that every FRAME spans the full exponent range
    along y, or is clustered, all denormals, the cell-boundary exponents, ties at 2^53, or has a sum that passes DBL_MAX (frame 5)."""
    return np.ascontiguousarray(meanref.synthetic_plane(seed, n, width).T)


def standard_bands(n):
    """The bands the feature's issue names for a plane of n rows: empty, one row, everything, a ragged run below 64 rows, 65 rows from
    row 3 (more than one load of 64), the last row, and two overlapping bands."""
    return [(0, 0), (0, 1), (0, n), (min(1, n), min(n, 64)), (min(n, 3), min(n, 3 + 65)), (n - 1, n), (0, n // 2 + 1), (n // 4, n)]
