"""Expected occupancy counts (include/spectroplot_hip.h, sp_plan_execute_occupancy): hit(x, y) = power[x][y] >= threshold[y] by numpy's
>=, counted per row over the frames and per band of rows and frame; and threshold vectors that plant what the compare can get wrong on
top of a plane (trackref.synthetic_plane's or any other).  Test infrastructure, not a test."""
import numpy as np

import meanref
import trackref

DENORMAL = 0x0000000000000001
NANS = (trackref.QUIET_NAN, trackref.NEGATIVE_NAN, trackref.SIGNALLING_NAN)
KINDS = 16      # the rotation of planted_thresholds


def hits(plane, threshold):
    """bool [width, n]: numpy's >= (a NaN on either side is no hit)."""
    plane = np.ascontiguousarray(plane, np.float64)
    t = np.asarray(threshold, np.float64)
    assert t.shape == (plane.shape[1],)
    with np.errstate(invalid="ignore"):
        return plane >= t[None, :]


def expected(plane, threshold, bands):
    """(rows uint32 [n], frames uint32 [count, width]) of a plane f64 [width, n] and thresholds f64 [n]."""
    h = hits(plane, threshold)
    rows = h.sum(axis=0, dtype=np.uint32)
    frames = np.zeros((len(bands), h.shape[0]), np.uint32)
    for b, (y0, y1) in enumerate(bands):
        frames[b] = h[:, y0:y1].sum(axis=1, dtype=np.uint32)
    return rows, frames


def assert_same(got, want, what=""):
    """got and want are (rows, frames), either of `got` may be None (not asked): equal words, with the first difference in words."""
    for name, g, w in zip(("rows", "frames"), got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.uint32 and g.shape == w.shape, "%s: %s %s %r, want %r" % (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        if len(bad):
            at = tuple(bad[0])
            raise AssertionError("%s: %s differ in %d of %d words, first at %r: got %r, want %r"
                                 % (what, name, len(bad), w.size, at, g[at], w[at]))


def planted_thresholds(plane, seed=0):
    """f64 [n] for a plane f64 [width, n].  Row y gets, by (y + seed) % KINDS:
      0  a value of that row of the plane itself (equality hits exist), 1 the bit pattern one above it, 2 the one below it;
      3 +0.0, 4 -0.0, 5 -1.0, 6 -inf, 7 +inf; 8 .. 10 the three NaN patterns of trackref; 11 the smallest denormal;
      12 .. 15 a value of trackref.PAIRS that differs from its partner only in the low or only in the high 32 bits (the plane plants
      both partners in frames 6 .. 8).
    The value taken from the plane is a finite positive one where the row has one."""
    plane = np.ascontiguousarray(plane, np.float64)
    width, n = plane.shape
    rng = np.random.default_rng(seed ^ 0x0cc)
    t = np.zeros(n)
    bits = t.view(np.uint64)
    pairs = [trackref.PAIRS[0][1], trackref.PAIRS[1][0], trackref.PAIRS[2][1], trackref.PAIRS[2][0]]
    for y in range(n):
        kind = (y + seed) % KINDS
        if kind < 3:
            col = plane[:, y] if width else np.zeros(0)
            good = col[np.isfinite(col) & (col > 0)]
            own = good[int(rng.integers(0, good.size))] if good.size else 1.0
            bits[y] = int(np.float64(own).view(np.uint64)) + (0, 1, -1)[kind]
        elif kind < 8:
            t[y] = (0.0, -0.0, -1.0, -np.inf, np.inf)[kind - 3]
        elif kind < 11:
            bits[y] = NANS[kind - 8]
        elif kind == 11:
            bits[y] = DENORMAL
        else:
            bits[y] = pairs[kind - 12]
    return t


def random_lists(seed, count):
    """`count` lists (values, thresholds, y0, y1) for sp_debug_occupancy: magnitudes over the full exponent range or clustered
    (meanref.random_values), NaNs of the three kinds and infs sprinkled over both; the thresholds are values of the list itself, their
    neighbouring bit patterns, other magnitudes, and the special values."""
    rng = np.random.default_rng(seed)
    special = np.array([0, 0x8000000000000000, 0xbff0000000000000, 0xfff0000000000000, 0x7ff0000000000000, DENORMAL, *NANS], np.uint64)
    out = []
    for i in range(count):
        n = int(rng.integers(1, 200))
        v = meanref.random_values(rng, n, clustered=bool(i % 3 == 1)).copy()
        t = meanref.random_values(rng, n, clustered=bool(i % 3 == 1)).copy()
        vb, tb = v.view(np.uint64), t.view(np.uint64)
        pick = rng.integers(0, 4, n)
        tb[pick == 0] = vb[pick == 0]                                              # equal
        ok = (v > 0) & np.isfinite(v)
        tb[(pick == 1) & ok] = vb[(pick == 1) & ok] + np.uint64(1)                  # one above, one below
        tb[(pick == 2) & ok] = vb[(pick == 2) & ok] - np.uint64(1)
        for a in (vb, tb):
            for y in rng.integers(0, n, int(rng.integers(0, 4))):
                a[y] = special[int(rng.integers(4 if a is vb else 0, len(special)))]   # (no negative value, any threshold)
        y0 = int(rng.integers(0, n + 1))
        y1 = int(rng.integers(y0, n + 1))
        if i % 5 == 0:
            y0, y1 = 0, n
        out.append((v, t, y0, y1))
    return out
