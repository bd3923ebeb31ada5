"""Expected per-bin min / max traces of a request (include/spectroplot_hip.h, sp_plan_execute_traces), from the EXISTING oracle only:
the dB plane of pyoracle.render(..., planes=True) folded along the columns with the worker's own `<` / `>` updates and start values
(lib/worker.js:82-83, 102-103), then permuted to image row order (worker.js:90).  Test infrastructure, not a test."""
import numpy as np

from oracle import pyoracle

_LUT = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)      # the colours do not reach a trace


def rows(n):
    """Image row y of bin i (worker.js:90)."""
    i = np.arange(n)
    return np.where(i <= n // 2, n // 2 - i, n // 2 + n - i)


def fold(db):
    """(trace_min, trace_max) in bin order of a dB plane [width, n], in order of x."""
    n = db.shape[1]
    tmin, tmax = np.full(n, 0.0), np.full(n, -200.0)
    with np.errstate(invalid="ignore"):
        for x in range(db.shape[0]):
            d = db[x]
            lo, hi = d < tmin, d > tmax          # a NaN compares false: it never wins
            tmin[lo] = d[lo]
            tmax[hi] = d[hi]
    return tmin, tmax


def expected(fmt, data, n, windowc, block_norm, gain, rng, width, channel_mode=False, columns=False):
    """{"trace_min": f64[n], "trace_max": f64[n]} in row order, and the oracle's "dBfs_min" / "dBfs_max" of the same request.
    columns: also "min_column" / "max_column", int [n] in bin order: the first frame that holds the bin's smallest / largest |X|^2."""
    ref = pyoracle.render(fmt, data, n, windowc, block_norm, gain, rng, _LUT, width, channel_mode, False, planes=True)
    tmin, tmax = fold(ref["db"])
    y = rows(n)
    out_min, out_max = np.empty(n), np.empty(n)
    out_min[y] = tmin
    out_max[y] = tmax
    out = {"trace_min": out_min, "trace_max": out_max, "dBfs_min": ref["dBfs_min"], "dBfs_max": ref["dBfs_max"]}
    if columns:
        out["min_column"], out["max_column"] = np.argmin(ref["abs2"], axis=0), np.argmax(ref["abs2"], axis=0)
    return out


def same_bits(a, b):
    """Bit-exact equality of two f64 arrays (-0.0 != 0.0, a NaN equals the same NaN)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def assert_same(got, want, what=""):
    for k in ("trace_min", "trace_max"):
        if not same_bits(got[k], want[k]):
            bad = np.flatnonzero(np.asarray(got[k]).view(np.uint64) != np.asarray(want[k]).view(np.uint64))
            raise AssertionError("%s: %s differs in %d of %d rows, first at row %d: got %r, want %r"
                                 % (what, k, len(bad), len(want[k]), bad[0], got[k][bad[0]], want[k][bad[0]]))
