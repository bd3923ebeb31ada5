"""Expected mean-power traces (include/spectroplot_hip.h, sp_plan_execute_mean): math.fsum of every column of a power plane - the
correctly rounded sum - divided by the width, with the NaN, inf and overflow rules of the header.  Test infrastructure, not a test."""
import math

import numpy as np


def exact_sum(values):
    """RN(exact sum) of non-negative doubles: any NaN gives NaN, else any +inf gives +inf, a sum that rounds past DBL_MAX gives +inf."""
    values = [float(v) for v in values]
    if any(v != v for v in values):
        return math.nan
    if any(v == math.inf for v in values):
        return math.inf
    try:
        return math.fsum(values)
    except OverflowError:
        return math.inf


def expected(plane):
    """f64[n]: mean[y] = exact_sum(plane[:, y]) / width for a plane f64 [width, n]; width == 0 gives NaN everywhere (0 / 0)."""
    plane = np.ascontiguousarray(plane, np.float64)
    width, n = plane.shape
    if width == 0:
        return np.full(n, np.nan)
    with np.errstate(all="ignore"):
        return np.array([exact_sum(plane[:, y]) for y in range(n)], np.float64) / np.float64(width)


def db_of(mean, block_norm, gain):
    """sp_plan_power_to_db of the means: (5 * log10(p) + block_norm_db + gain) - gain in that order (lib/worker.js:93, 100), log10 the
    oracle's restatement of the engine's."""
    from oracle import pyoracle
    log10 = pyoracle.lib().spo_log10
    block_norm_db = 10 * log10(float(block_norm))
    return np.array([(5 * log10(float(p)) + block_norm_db + gain) - gain for p in mean], np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    """Two f64 arrays agree: the same shape, NaN at the same places (a NaN is any NaN), the same bits everywhere else."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (bits(a)[~na] == bits(b)[~na]).all())


def assert_same(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    if same(got, want):
        return
    na, nb = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((na != nb) | (~na & ~nb & (bits(got) != bits(want))))
    y = bad[0]
    raise AssertionError("%s: the mean differs in %d of %d rows, first at row %d: got %r, want %r"
                         % (what, len(bad), want.size, y, got[y], want[y]))


def _from_fields(rng, e, count):
    m = rng.integers(0, 1 << 52, count, dtype=np.uint64)
    return ((np.asarray(e, np.uint64) << np.uint64(52)) | m).view(np.float64)


def random_values(rng, count, clustered=False):
    """`count` non-negative finite doubles: exponent fields over the whole range [0, 2046] (denormals included), or within 4 of each
    other; now and then a significand of all ones, all zeros or a single low bit (ties and sticky bits)."""
    if clustered:
        e0 = int(rng.integers(0, 2044))
        e = rng.integers(e0, e0 + 4, count)
    else:
        e = rng.integers(0, 2047, count)
    v = _from_fields(rng, e, count).copy()
    b = v.view(np.uint64)
    pick = rng.integers(0, 8, count)
    b[pick == 0] &= np.uint64(0xfff0000000000000)
    b[pick == 1] |= np.uint64(0x000fffffffffffff)
    b[pick == 2] = (b[pick == 2] & np.uint64(0xfff0000000000000)) | np.uint64(1)
    return v


def boundary_values():
    """One value with a full significand at every exponent whose shift within a cell is 0, 1, 30 or 31, in the cells 0, 1, 62 and 63."""
    out = []
    for cell in (0, 1, 62, 63):
        for s in (0, 1, 30, 31):
            e = 32 * cell + s + 1
            if e <= 2046:
                out.append(np.array([(e << 52) | 0x000fffffffffffff], np.uint64).view(np.float64)[0])
    return out


def synthetic_plane(seed, width, n):
    """A plane f64 [width, n] of non-negative finite values for sp_power_mean: rows over the full exponent range, clustered rows,
    denormal rows, the cell-boundary exponents, ties at 2^53, and a row whose sum passes DBL_MAX."""
    rng = np.random.default_rng(seed)
    plane = np.empty((width, n))
    edge = boundary_values()
    for y in range(n):
        k = y % 6
        if k == 0:
            col = random_values(rng, width)
        elif k == 1:
            col = random_values(rng, width, clustered=True)
        elif k == 2:
            col = _from_fields(rng, np.zeros(width, np.int64), width)                 # denormals
        elif k == 3:
            col = np.array([edge[(y + x) % len(edge)] for x in range(width)])
        elif k == 4:
            col = np.array([[2.0 ** 53, 1.0, 5e-324, 3.0, 0.0][(x + y // 6) % 5] for x in range(width)])
        else:
            col = np.full(width, np.finfo(np.float64).max)
        plane[:, y] = col
    return plane
