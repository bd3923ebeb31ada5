"""Expected lagged covariance sums (include/spectroplot_hip.h, sp_plan_execute_lagcov): for two series a and b of `width` non-negative
doubles and the lags [0, lags), with N = width - lags + 1 terms (0 where that is below 1), the exact P = sum a[x] * b[x + l],
A = sum a[x] and B = sum b[x + l] over x in [0, N) and the three results float(P), float(N * P - A * B), float(B), each rounded once by
float(Fraction) - round to nearest, ties to even, correctly into the denormal range, OverflowError read as the infinity of the value's
sign.  Every double is scaled to a Python integer in units of 2^-1074, so the products and the difference are integers.  The special
value rule goes by window membership: a NaN among a[0 .. N) and b[l .. l + N) gives NaN in all three, otherwise a +inf among them gives
+inf.  Nothing here uses the code under test.  Test infrastructure, not a test."""
import math
from fractions import Fraction

import numpy as np

UNIT = Fraction(1, 2 ** 1074)
UNIT2 = UNIT * UNIT


def _round(q):
    try:
        return float(q)
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def scaled(values):
    """The finite values as Python integers in units of 2^-1074 (an object array; a NaN or an inf becomes 0), exactly."""
    values = np.ascontiguousarray(values, np.float64)
    out = np.zeros(values.size, object)
    for k, v in enumerate(values.tolist()):
        if v == v and v != math.inf and v:
            num, den = abs(v).as_integer_ratio()            # den is a power of two, at most 2^1074
            out[k] = num * (2 ** 1074 // den)
    return out


def pair(a, b, lags):
    """f64 [3, lags] of the series a and b (equally long)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape and a.ndim == 1 and lags >= 1
    width = a.size
    n = max(width - lags + 1, 0)
    out = np.zeros((3, lags), np.float64)
    if n == 0:
        return out
    ia, ib = scaled(a), scaled(b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    inf_a, inf_b = np.isinf(a), np.isinf(b)
    sum_a = int(ia[:n].sum())
    for l in range(lags):
        if nan_a[:n].any() or nan_b[l:l + n].any():
            out[:, l] = math.nan
        elif inf_a[:n].any() or inf_b[l:l + n].any():
            out[:, l] = math.inf
        else:
            wb = ib[l:l + n]
            p, sum_b = int((ia[:n] * wb).sum()), int(wb.sum())
            out[0, l] = _round(Fraction(p) * UNIT2)
            out[1, l] = _round(Fraction(n * p - sum_a * sum_b) * UNIT2)     # (an exact zero is +0.0; a negative one below the grid -0.0)
            out[2, l] = _round(Fraction(sum_b) * UNIT)
    return out


def expected(series, pairs, lags):
    """f64 [3, npairs, lags] for a band-major series f64 [count, width] and the index pairs."""
    series = np.ascontiguousarray(series, np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = np.zeros((3, len(pairs), lags), np.float64)
    for k, (i, j) in enumerate(pairs):
        out[:, k, :] = pair(series[i], series[j], lags)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, want, what=""):
    """NaN at the same places (a NaN is any NaN), the same bits - the sign of a zero included - everywhere else."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), "%s: NaN at %r, want at %r" % (what, np.argwhere(gn != wn)[:4].tolist(), int(wn.sum()))
    bad = (bits(got) != bits(want)) & ~wn
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d differ, first at %r: got %r, want %r" % (what, int(bad.sum()), got.size, at, got[at], want[at]))


def _f(pattern):
    return np.array([pattern], np.uint64).view(np.float64)[0]


def from_fields(rng, e, count):
    """`count` doubles with the exponent fields e and random fractions."""
    frac = rng.integers(0, 1 << 52, count, dtype=np.uint64)
    return ((np.asarray(e, np.uint64) << np.uint64(52)) | frac).view(np.float64)


def full_range(rng, count):
    """Doubles over the whole exponent range, denormals and DBL_MAX's exponent included, a few zeros among them."""
    v = from_fields(rng, rng.integers(0, 2047, count), count)
    v[rng.random(count) < 0.1] = 0.0
    return v


def clustered(rng, count, pedestal=1.0):
    """A series on a pedestal: what a band-power series looks like."""
    return pedestal * (1.0 + 1e-3 * rng.random(count))


def pedestal_series(width=257):
    """The issue's example: 1e6 + 1e-6 * square(period 8) + 1e-9 * noise."""
    rng = np.random.default_rng(8)
    x = np.arange(width)
    return 1e6 + 1e-6 * ((x // 4) % 2).astype(np.float64) + 1e-9 * rng.random(width)


def synthetic_series(seed, count, width):
    """f64 [count, width]: band 0 on a pedestal with a period, band 1 its complement (a negative cross-covariance), band 2 over the
    full exponent range, band 3 with zeros and denormals, the others clustered at powers far apart."""
    rng = np.random.default_rng(seed)
    s = np.zeros((count, width), np.float64)
    x = np.arange(width)
    for b in range(count):
        k = b % 6
        if k == 0:
            s[b] = 1e3 + ((x // 3) % 2) * 0.25 + 1e-7 * rng.random(width)
        elif k == 1:
            s[b] = 1e3 + (1 - (x // 3) % 2) * 0.25 + 1e-7 * rng.random(width)
        elif k == 2:
            s[b] = full_range(rng, width)
        elif k == 3:
            s[b] = from_fields(rng, np.zeros(width, np.int64), width)
            s[b][rng.random(width) < 0.3] = 0.0
        elif k == 4:
            s[b] = clustered(rng, width, 1e-150)
        else:
            s[b] = clustered(rng, width, 1e150)
    return s
