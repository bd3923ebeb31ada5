"""Expected averaged spectrograms (include/spectroplot_hip.h, sp_plan_execute_blockmean): math.fsum of every column's frames of a power
plane, per row - the correctly rounded sum - divided by the column's number of frames, with the NaN, inf and overflow rules of the
mean-power trace.  Test infrastructure, not a test."""
import math

import numpy as np

import meanref

NAN_BITS = 0x7ff8000000000000
DBL_MAX = float(np.finfo(np.float64).max)
TINY = 5e-324


def columns(width, group):
    """ceil(width / group); 0 where width <= 0 or group < 1."""
    return 0 if width <= 0 or group < 1 else -(-int(width) // int(group))


def expected(plane, group):
    """f64 [columns, n]: out[c, y] = exact_sum(plane[c * group : (c + 1) * group, y]) / count_c for a plane f64 [width, n]; every NaN is
    the one NaN 0x7ff8000000000000."""
    plane = np.ascontiguousarray(plane, np.float64)
    width, n = plane.shape
    cols = columns(width, group)
    out = np.empty((cols, n), np.float64)
    with np.errstate(all="ignore"):
        for c in range(cols):
            part = plane[c * group:min((c + 1) * group, width)]
            sums = np.array([meanref.exact_sum(part[:, y]) for y in range(n)], np.float64)
            out[c] = sums / np.float64(part.shape[0])
    out.view(np.uint64)[np.isnan(out)] = NAN_BITS
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, want, what=""):
    """Bit for bit, the NaNs too: a block mean's NaN is the one NaN."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    if len(bad):
        c, y = bad[0]
        raise AssertionError("%s: %d of %d values differ, first at column %d, row %d: got %r (%016x), want %r (%016x)"
                             % (what, len(bad), want.size, c, y, got[c, y], bits(got)[c, y], want[c, y], bits(want)[c, y]))


# --- the resident plane of the GPU test: meanref's synthetic plane with the cases of the issue planted in single columns of group 5 ---
WIDTH, N, PLANT_GROUP = 131, 96, 5          # 131 = 26 * 5 + 1: a one-frame last column; n = 96: two bands of 64 rows, the second half empty
PLANTS = {                                  # name: (row, column of group 5, the column's five frames)
    "sticky": (6, 2, [2.0 ** 53, 1.0, TINY, 0.0, 0.0]),
    "tie": (7, 3, [2.0 ** 53, 1.0, 0.0, 0.0, 0.0]),
    "far apart": (8, 4, [1e300, 0.0, 1e-300, 0.0, 0.0]),
    "overflow": (9, 5, [DBL_MAX, 0.0, 0.0, DBL_MAX, 0.0]),
    "nan": (10, 6, [1.0, 1.0, math.nan, 1.0, 1.0]),
    "inf": (11, 7, [1.0, math.inf, 1.0, 1.0, 1.0]),
    "zeros": (12, 8, [0.0] * 5),
    "denormals": (13, 9, [TINY, 3 * TINY, 2.0 ** -1040, 0.0, 7 * TINY]),
}


def planted_plane(seed=20261021):
    plane = meanref.synthetic_plane(seed, WIDTH, N)
    for row, col, values in PLANTS.values():
        plane[:, row] = 1.0 + (np.arange(WIDTH) % 3)
        plane[col * PLANT_GROUP:(col + 1) * PLANT_GROUP, row] = values
    return plane


def telling(plane):
    """The planted cases are really there: asserted on the EXPECTED arrays, not on anything the library made."""
    e = expected(plane, PLANT_GROUP)
    assert e.shape == (27, N) and columns(WIDTH, PLANT_GROUP) == 27
    at = {name: e[col, row] for name, (row, col, _) in PLANTS.items()}
    assert at["sticky"] == (2.0 ** 53 + 2) / 5 and at["tie"] == 2.0 ** 53 / 5 and at["far apart"] == 1e300 / 5
    assert at["overflow"] == math.inf and at["inf"] == math.inf
    assert bits(e)[PLANTS["nan"][1], PLANTS["nan"][0]] == NAN_BITS
    assert bits(e)[PLANTS["zeros"][1], PLANTS["zeros"][0]] == 0
    assert 0 < at["denormals"] < 2.0 ** -1022
    for name in ("nan", "inf", "overflow"):
        row, col, _ = PLANTS[name]
        assert np.isfinite(e[col - 1, row]) and np.isfinite(e[col + 1, row]), name   # the neighbouring columns stay finite
    # the last column is one frame, and it is that frame
    assert (bits(e)[26] == bits(plane)[130]).all()
    # group 1 is the plane, a group of the whole width the mean
    assert (bits(expected(plane, 1)) == bits(plane)).all()   # (the planted NaN is the one NaN already)
    for group in (WIDTH, WIDTH + 1, 1000):
        assert meanref.same(expected(plane, group)[0], meanref.expected(plane)) and expected(plane, group).shape == (1, N)
    return e
