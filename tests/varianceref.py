"""Expected variance sums (include/spectroplot_hip.h, sp_plan_execute_variance): per row of a power plane, over its W frames, the exact
rational S1 = sum p and S2 = sum p**2 and the three results float(S1), float(S2), float(W * S2 - S1**2), each rounded once by float()
- round to nearest, ties to even, correctly into the denormal range - with the mean's special value rule on all three (any NaN gives
NaN, else any +inf gives +inf) and OverflowError read as +inf.  Nothing here uses the code under test.  Test infrastructure, not a
test."""
import math
from fractions import Fraction

import numpy as np

import meanref


def _round(q):
    try:
        return float(q)
    except OverflowError:
        return math.inf


def column(values):
    """f64 [3] of one row's values over W = len(values) frames."""
    values = [float(v) for v in values]
    if any(v != v for v in values):
        return np.full(3, math.nan)
    if any(v == math.inf for v in values):
        return np.full(3, math.inf)
    fr = [Fraction(v) for v in values if v]
    s1, s2 = sum(fr, Fraction(0)), sum((f * f for f in fr), Fraction(0))
    d = len(values) * s2 - s1 * s1
    assert d >= 0
    return np.array([_round(s1), _round(s2), _round(d)], np.float64)


def dense_column(values):
    """column() for a long row, exact all the same: every value is an integer m times 2^e (np.frexp), the sums are integer sums of
    m << (e - emin) and of m * m << 2 (e - emin) in Python integers (numpy object arrays), rounded once by float(Fraction)."""
    values = np.ascontiguousarray(values, np.float64)
    if np.isnan(values).any():
        return np.full(3, math.nan)
    if np.isinf(values).any():
        return np.full(3, math.inf)
    rows = np.flatnonzero(values)
    if not rows.size:
        return np.zeros(3)
    frac, e = np.frexp(values[rows])
    m = (frac * 2.0 ** 53).astype(np.int64)                      # exact: at most 53 significant bits
    assert ((m.astype(np.float64) * 2.0 ** -53) == frac).all()
    e = e.astype(np.int64) - 53
    emin = int(e.min())
    scaled = np.left_shift(m.astype(object), (e - emin).astype(object))
    s1, s2 = int(scaled.sum()), int((scaled * scaled).sum())
    d = values.size * s2 - s1 * s1
    assert d >= 0
    unit = Fraction(2) ** emin
    return np.array([_round(Fraction(s1) * unit), _round(Fraction(s2) * unit * unit), _round(Fraction(d) * unit * unit)], np.float64)


def expected(plane):
    """f64 [3, n] for a plane f64 [width, n]; width == 0 gives zeros."""
    plane = np.ascontiguousarray(plane, np.float64)
    width, n = plane.shape
    out = np.zeros((3, n), np.float64)
    for y in range(n):
        out[:, y] = dense_column(plane[:, y]) if width > 64 else column(plane[:, y])
    return out


def assert_same(got, want, what=""):
    """meanref.assert_same's comparison - NaN at the same places (a NaN is any NaN), the same bits everywhere else - array by array."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    if got.ndim == 1:
        return meanref.assert_same(got, want, what)
    for k, name in enumerate(("sum", "sum of squares", "W * S2 - S1^2")):
        meanref.assert_same(got[k], want[k], "%s, %s" % (what, name))


def _f(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def one_ulp_up(v):
    return _f(int(np.array([v], np.float64).view(np.uint64)[0]) + 1)


def columns():
    """(name, values) of the rows the CPU tests feed sp_debug_variance_sums and the stand-alone program: the full exponent range, all
    denormals, squares that land in the denormal range and below it, ties there, every cell-boundary shift - an odd and an even
    e - 1 of each pair whose squares share a cell - DBL_MAX twice, constant rows, one-ulp rows and special values."""
    rng = np.random.default_rng(20250)
    big, tiny = np.finfo(np.float64).max, 5e-324
    full = 0x000fffffffffffff
    cols = [("empty", []), ("one value", [3.5]), ("zeros", [0.0] * 5), ("one two three", [1.0, 2.0, 3.0]),
            ("full range", meanref.random_values(rng, 300)), ("clustered", meanref.random_values(rng, 200, clustered=True)),
            ("clustered, long", meanref.random_values(rng, 1500, clustered=True)),
            ("denormals", meanref._from_fields(rng, np.zeros(130, np.int64), 130)),
            ("squares around the denormal grid", meanref._from_fields(rng, rng.integers(440, 520, 90), 90)),
            ("square of 2^-537, twice", [2.0 ** -537] * 2), ("square of 2^-538: a quarter of a denormal", [2.0 ** -538]),
            ("below the half step", [2.0 ** -537, 2.0 ** -538]), ("tie in the denormal grid, up", [2.0 ** -537] + [2.0 ** -538] * 2),
            ("tie in the denormal grid, down", [2.0 ** -537] * 2 + [2.0 ** -538] * 2),
            ("just above the tie", [2.0 ** -537, 2.0 ** -538, 2.0 ** -538, tiny]), ("the tie at zero", [2.0 ** -538] * 2),
            ("largest denormal square", [one_ulp_up(2.0 ** -512), 2.0 ** -520]), ("smallest normal square", [2.0 ** -511, 2.0 ** -530]),
            ("1e200", [1e200]), ("DBL_MAX", [big]), ("DBL_MAX twice", [big, big]), ("DBL_MAX and a denormal", [big, tiny, big, 1.0]),
            ("tie to even at 2^53", [3.0, 2.0 ** 53 + 2, 0.5]),
            ("nan first", [math.nan, 1.0, 2.0]), ("inf first", [math.inf, 1.0, 2.0]), ("nan elsewhere", [1.0, 2.0, math.nan, 4.0]),
            ("nan beats inf", [math.inf, 1.0, math.nan]), ("inf alone", [math.inf]),
            ("boundary values", meanref.boundary_values())]
    for length in (1, 2, 1000):
        cols.append(("constant, %d" % length, [0.1] * length))
    v = 1234.5678e-3
    cols.append(("constant but one ulp", [v] * 999 + [one_ulp_up(v)]))
    cols.append(("constant but one ulp, two frames", [v, one_ulp_up(v)]))
    for cell in (0, 1, 31, 62, 63):
        for shift in (0, 1, 15, 16, 30, 31):     # (e - 1) % 32: 15 and 16 are the odd / even pair around the squared cell's boundary
            e = 32 * cell + shift + 1
            if e <= 2046:
                v = _f((e << 52) | full)
                cols.append(("cell %d shift %d" % (cell, shift), [v, v, _f(e << 52), v, _f((e << 52) | 1)] * 13))
    return [(name, np.array(v, np.float64)) for name, v in cols]


def synthetic_plane(seed, width, n):
    """meanref.synthetic_plane - the full exponent range, clustered rows, denormals, cell-boundary exponents, a row of DBL_MAX - with
    rows of the kinds the variance is about laid over it: constant rows, rows constant but for one ulp in one frame, one frame of
    DBL_MAX in a quiet row, and a NaN row, an inf row and a row with both."""
    rng = np.random.default_rng(seed + 77)
    plane = meanref.synthetic_plane(seed, width, n)
    for y in range(n):
        k = y % 16
        if k == 7:
            plane[:, y] = rng.random() + 0.5
        elif k == 8:
            plane[:, y] = v = rng.random() * 1e-3 + 1e-6
            plane[int(rng.integers(0, width)), y] = one_ulp_up(v)
        elif k == 9:
            plane[:, y] = rng.random(width) * 1e-9
            plane[int(rng.integers(0, width)), y] = np.finfo(np.float64).max
        elif k == 13:
            plane[int(rng.integers(0, width)), y] = math.nan
        elif k == 14:
            plane[int(rng.integers(0, width)), y] = math.inf
        elif k == 15 and width > 1:
            plane[0, y], plane[width - 1, y] = math.inf, math.nan
    return plane
