"""Expected spectral moments (include/spectroplot_hip.h, sp_plan_execute_moments): per band, frame and k the exact rational sum of
(y - y0)**k * power[x][y] over the band's rows, rounded once by float() - round to nearest, ties to even - with the header's special
value rule (a band's NaN or +inf marks EVERY moment, whatever the row's weight) and OverflowError read as +inf.  Nothing here uses the
code under test.  Test infrastructure, not a test."""
import math
from fractions import Fraction

import numpy as np

import bandref
import meanref

MAX_ORDER = 2


def weighted_sum(values, k):
    """RN(sum of r**k * values[r]) over one column of non-negative doubles, r = 0 .. len - 1 and 0**0 = 1: any NaN gives NaN, else any
    +inf gives +inf - also at weight 0 - and a sum that rounds past DBL_MAX gives +inf."""
    values = [float(v) for v in values]
    if any(v != v for v in values):
        return math.nan
    if any(v == math.inf for v in values):
        return math.inf
    total = sum((Fraction(r ** k) * Fraction(v) for r, v in enumerate(values) if v), Fraction(0))
    try:
        return float(total)
    except OverflowError:
        return math.inf


def column(values, order=MAX_ORDER):
    """f64 [order + 1]: the moments 0 .. order of one column."""
    return np.array([weighted_sum(values, k) for k in range(order + 1)], np.float64)


def expected(plane, bands, order=MAX_ORDER):
    """f64 [order + 1, count, width]: out[k, b, x] = weighted_sum(plane[x, y0_b:y1_b], k) for a plane f64 [width, n]; an empty band
    gives +0.0 in every moment."""
    plane = np.ascontiguousarray(plane, np.float64)
    width = plane.shape[0]
    out = np.zeros((order + 1, len(bands), width), np.float64)
    for b, (y0, y1) in enumerate(bands):
        for x in range(width):
            out[:, b, x] = column(plane[x, y0:y1], order)
    return out


def assert_same(got, want, what=""):
    """bandref.assert_same's comparison - the same shape, NaN at the same places (a NaN is any NaN), the same bits everywhere else - of
    two moment arrays [order + 1, count, width], moment by moment."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    for k in range(want.shape[0]):
        bandref.assert_same(got[k], want[k], "%s, moment %d" % (what, k))


def _f(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def columns():
    """(name, values) of the columns the CPU tests feed sp_debug_moment_sum and the stand-alone program: the full exponent range, all
    denormals, every cell-boundary shift, the two ties, DBL_MAX, and special values in row 0 and elsewhere."""
    rng = np.random.default_rng(20240)
    big, tiny = np.finfo(np.float64).max, 5e-324
    full = 0x000fffffffffffff
    cols = [("empty", []), ("one row", [3.5]), ("zeros", [0.0] * 5),
            ("full range", meanref.random_values(rng, 300)), ("clustered", meanref.random_values(rng, 200, clustered=True)),
            ("denormals", meanref._from_fields(rng, np.zeros(130, np.int64), 130)),
            ("tie to even, up", [3.0, 2.0 ** 53 + 2, 0.5]), ("tie to even, down", [3.0, 2.0 ** 53, 0.5]),
            ("DBL_MAX at weight 2", [0.0, 0.0, big]), ("DBL_MAX at weight 1", [0.0, big]), ("DBL_MAX in row 0", [big, 1.0, 2.0]),
            ("DBL_MAX twice", [big, big]), ("smallest denormal at weight 1024", [0.0] * 1024 + [tiny]),
            ("nan in row 0", [math.nan, 1.0, 2.0]), ("inf in row 0", [math.inf, 1.0, 2.0]), ("nan elsewhere", [1.0, 2.0, math.nan, 4.0]),
            ("inf elsewhere", [1.0, math.inf, 3.0]), ("nan beats inf", [math.inf, 1.0, math.nan]), ("inf alone", [math.inf]),
            ("boundary values", meanref.boundary_values())]
    for cell in (0, 1, 31, 62, 63):
        for shift in (0, 11, 12, 31):        # (e - 1) % 32: 12 is the first shift whose unweighted value needs a third piece
            e = 32 * cell + shift + 1
            if e <= 2046:
                v = _f((e << 52) | full)
                cols.append(("cell %d shift %d" % (cell, shift), [v, v, _f(e << 52), v, _f((e << 52) | 1)] * 13))
    return [(name, np.array(v, np.float64)) for name, v in cols]


def last_row_column(n=1 << 20):
    """A column of n rows whose one value stands in the last row: the largest weight."""
    v = np.zeros(n, np.float64)
    v[n - 1] = _f((1000 << 52) | 0x000fffffffffffff)
    return v


def last_row_expected(values):
    """column() of a column that is zero but for some rows, without walking the zeros."""
    out = []
    for k in range(MAX_ORDER + 1):
        total = sum((Fraction(int(r) ** k) * Fraction(float(values[r])) for r in np.flatnonzero(values)), Fraction(0))
        try:
            out.append(float(total))
        except OverflowError:
            out.append(math.inf)
    return np.array(out, np.float64)


def dense_column(values, order=MAX_ORDER):
    """column() for a long column, exact all the same: every value is an integer m times 2^e (np.frexp), the weighted sum an integer
    sum of (r**k * m) << (e - emin) in Python integers (numpy object arrays), rounded once by float(Fraction)."""
    values = np.ascontiguousarray(values, np.float64)
    if np.isnan(values).any():
        return np.full(order + 1, math.nan)
    if np.isinf(values).any():
        return np.full(order + 1, math.inf)
    rows = np.flatnonzero(values)
    if not rows.size:
        return np.zeros(order + 1)
    frac, e = np.frexp(values[rows])
    m = (frac * 2.0 ** 53).astype(np.int64)                      # exact: at most 53 significant bits
    assert ((m.astype(np.float64) * 2.0 ** -53) == frac).all()
    e = e.astype(np.int64) - 53
    emin = int(e.min())
    scaled = np.left_shift(m.astype(object), (e - emin).astype(object))
    r = rows.astype(object)
    out = []
    for k in range(order + 1):
        total = int((scaled * r ** k).sum()) if k else int(scaled.sum())
        try:
            out.append(float(Fraction(total) * Fraction(2) ** emin))
        except OverflowError:
            out.append(math.inf)
    return np.array(out, np.float64)
