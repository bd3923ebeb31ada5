"""Expected peak tracks (include/spectroplot_hip.h, sp_plan_execute_track): per band of image rows and per frame of a power plane the
strongest row that is not a NaN - the smallest among equal ones - and its value, by numpy's argmax, which returns the first of equal
maxima; and planes that plant the ties, the neighbouring bit patterns and the NaN / inf cases the comparison can get wrong.  Test
infrastructure, not a test."""
import numpy as np

import bandref
import meanref

DBL_MAX = float(np.finfo(np.float64).max)
QUIET_NAN, NEGATIVE_NAN, SIGNALLING_NAN = 0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000001
TIE_FRAMES, PAIR_FRAMES, SPECIAL_FRAMES = 6, 5, 6
# the pairs of frames 6 .. 10 as bit patterns (smaller, larger): they differ only in the low 32 bits, only in the high 32 bits, with
# the larger low word on the smaller value, DBL_MAX against +inf, +0.0 against the smallest denormal
PAIRS = [(0x4000000000000001, 0x4000000000000002), (0x4000000100000000, 0x4000000200000000), (0x40000001ffffffff, 0x4000000200000000),
         (0x7fefffffffffffff, 0x7ff0000000000000), (0x0000000000000000, 0x0000000000000001)]


def frame_peak(p, y0):
    """(row, peak) of one band's values p = plane[x, y0:y1] by the header's numpy rule."""
    p = np.asarray(p, np.float64)
    if p.size == 0 or np.isnan(p).all():
        return -1, np.nan
    k = int(np.argmax(np.where(np.isnan(p), -1.0, p)))
    return y0 + k, p[k]


def expected(plane, bands):
    """(rows int32 [count, width], peaks f64 [count, width]) of a plane f64 [width, n]."""
    plane = np.ascontiguousarray(plane, np.float64)
    width = plane.shape[0]
    rows, peaks = np.full((len(bands), width), -1, np.int32), np.full((len(bands), width), np.nan)
    for b, (y0, y1) in enumerate(bands):
        p = plane[:, y0:y1]
        if p.shape[1] == 0 or width == 0:
            continue
        nan = np.isnan(p)
        k = np.argmax(np.where(nan, -1.0, p), axis=1)
        some = ~nan.all(axis=1)
        rows[b, some] = (y0 + k)[some]
        peaks[b, some] = p[np.arange(width), k][some]
    return rows, peaks


def assert_same(got, want, what=""):
    """got and want are (rows, peaks): the rows equal, the peaks NaN at the same places (a NaN is any NaN) and the same bits elsewhere,
    with the first difference in words."""
    (g_rows, g_peaks), (w_rows, w_peaks) = got, want
    g_rows, w_rows = np.asarray(g_rows), np.asarray(w_rows)
    assert g_rows.dtype == np.int32 and g_rows.shape == w_rows.shape, "%s: rows %s %r, want %r" % (what, g_rows.dtype, g_rows.shape, w_rows.shape)
    bad = np.argwhere(g_rows != w_rows)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: the rows differ in %d of %d values, first at (band, frame) %r: got %r, want %r"
                             % (what, len(bad), w_rows.size, at, g_rows[at], w_rows[at]))
    bandref.assert_same(g_peaks, w_peaks, what + " (peaks)")


def synthetic_plane(seed, n, width):
    """A plane f64 [width, n] for sp_power_tracks on top of bandref.synthetic_plane (frames over the full exponent range, clustered,
    denormal, at the cell boundaries, repeating five values, all DBL_MAX).  Where the width allows:
    frames 0 .. 5 plant ties - the maximum twice in rows 5 and 6; in rows 5 and 69 (the same lane of two loads); in rows 8 and 69 (the
      later load holds the smaller lane); all rows equal; all rows +0.0; a maximum in row 0 equal to one in row n - 1 (rows modulo n);
    frames 6 .. 10 pair two values whose order a 32-bit or a floating-point compare gets wrong (PAIRS), the larger one alternately in
      the later and in the earlier row;
    frames 11 .. 16 get, on top of what they hold: a quiet NaN; a NaN with the sign bit set; the signalling pattern one above +inf's
      (each larger as a bit pattern than every value of its frame); rows 1 .. 63 all NaN; an inf that must win; an inf with a NaN on
      either side that must not."""
    rng = np.random.default_rng(seed ^ 0x7ac)
    plane = bandref.synthetic_plane(seed, n, width).copy()
    bits = plane.view(np.uint64)
    r = lambda k: k % n  # noqa: E731
    ties = [(r(5), r(6)), (r(5), r(69)), (r(8), r(69)), None, None, (0, n - 1)]
    for x in range(min(width, TIE_FRAMES)):
        plane[x] = rng.random(n)                         # below 1.0
        if x == 3:
            plane[x] = 1.5
        elif x == 4:
            plane[x] = 0.0
        else:
            for y in ties[x]:
                plane[x, y] = 2.0
    p, q = n // 3, n - 1 - n // 5                        # p < q for every n >= 2
    for j, (small, large) in enumerate(PAIRS):
        x = TIE_FRAMES + j
        if x >= width:
            break
        plane[x] = 0.0 if j == 4 else rng.random(n)
        a, b = (p, q) if x % 2 == 0 else (q, p)
        bits[x, a], bits[x, b] = small, large
    x0 = TIE_FRAMES + PAIR_FRAMES
    mid = n // 2
    for j in range(SPECIAL_FRAMES):
        x = x0 + j
        if x >= width:
            break
        if j < 3:
            bits[x, mid] = (QUIET_NAN, NEGATIVE_NAN, SIGNALLING_NAN)[j]
        elif j == 3:
            plane[x, 1:min(n, 64)] = np.nan
        elif j == 4:
            plane[x, mid] = np.inf
        else:
            plane[x, mid] = np.inf
            bits[x, mid - 1] = SIGNALLING_NAN
            if mid + 1 < n:
                bits[x, mid + 1] = NEGATIVE_NAN
    return plane


def random_lists(seed, count):
    """`count` lists (values, y0, y1) for sp_debug_band_peak: magnitudes over the full exponent range or clustered (meanref), with
    duplicated maxima and NaNs of all three kinds at random places, now and then an inf or nothing but NaN."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(1, 200))
        v = meanref.random_values(rng, n, clustered=bool(i % 3 == 1)).copy()
        b = v.view(np.uint64)
        kind = i % 8
        if kind in (1, 2, 5) and n > 1:                  # the maximum once or twice more
            top = v.max()
            v[rng.integers(0, n, int(rng.integers(1, 3)))] = top
        if kind in (2, 3, 4):                            # NaNs, of every kind
            for y in rng.integers(0, n, int(rng.integers(1, 4))):
                b[y] = (QUIET_NAN, NEGATIVE_NAN, SIGNALLING_NAN)[int(rng.integers(0, 3))]
        if kind == 6:
            v[rng.integers(0, n, 2)] = np.inf
        if kind == 7 and i % 16 == 7:
            b[:] = NEGATIVE_NAN
        y0 = int(rng.integers(0, n + 1))
        y1 = int(rng.integers(y0, n + 1))
        if i % 5 == 0:
            y0, y1 = 0, n
        out.append((v, y0, y1))
    return out
