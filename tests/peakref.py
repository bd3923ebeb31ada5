"""Expected replies of the peak detector (include/spectroplot_hip.h, enum sp_detector), built from the EXISTING oracle only.

Sub-frame plane j of a request is pyoracle.render(..., planes=True) on the capture shifted by j * n samples with j * n zero samples
appended: byte length, sampleCount, stride and every p(x) are unchanged, and frame x of that call is sub-frame j of column x.  The planes
are masked by the existence rule, folded with the fmax rule in order of j, and the winning plane j* per pixel supplies the pixel: its
colour index (read back through an injective LUT), its dB value for cB_hist, the column's and the request's dBfs range and the two
gauges, restated here in integer / clamp arithmetic.  gauge_amps comes from plane 0.  Test infrastructure, not a test.
"""
import numpy as np

from oracle import pyoracle

SW = {"CU4": 1, "CS4": 1, "CU8": 2, "CS8": 2, "CU12": 3, "CS12": 3, "CU16": 4, "CS16": 4, "CU32": 8, "CS32": 8, "CU64": 16, "CS64": 16,
      "CF32": 8, "CF64": 16}
FORMATS = ["CU4", "CS4", "CU8", "CS8", "CU12", "CS12", "CU16", "CS16", "CU32", "CS32", "CU64", "CS64", "CF32", "CF64"]


def to_int32(v):
    """JS ~~v for the values that occur here."""
    if not np.isfinite(v):
        return 0
    r = int(np.trunc(v)) & 0xFFFFFFFF
    return r - (1 << 32) if r >= (1 << 31) else r


def subframe_rule(fmt, n, nbytes, width):
    """(M, counts[width]) by the issue's rule in JS arithmetic: M sub-frames per column, how many of them exist in each column."""
    sample_count = nbytes / SW[fmt.upper()]
    if width < 1:
        return 1, []
    with np.errstate(all="ignore"):
        stride = (np.float64(sample_count) - n) / np.float64(width - 1)
    M = int(np.floor(stride / n)) if (width >= 2 and np.isfinite(stride) and stride >= 2 * n) else 1
    counts = []
    for x in range(width):
        with np.errstate(all="ignore"):
            p = to_int32(0.5 + stride * x)
        c = 1
        for j in range(1, M):
            if p + (j + 1) * n <= sample_count:
                c = j + 1
            else:
                break
        counts.append(c)
    return M, counts


def _clamp_u8(v):
    v = np.asarray(v, dtype=np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.rint(np.clip(v, 0.0, 255.0)).astype(np.uint8)


def _pixel_offsets(n, width, waterfall):
    i = np.arange(n)
    y = np.where(i <= n // 2, n // 2 - i, n // 2 + n - i)
    x = np.arange(width)[:, None]
    if waterfall:
        return (n * (width - 1 - x) + (n - 1 - y)[None, :]) * 4
    return (x + width * y[None, :]) * 4


def expected(fmt, data, n, windowc, block_norm, gain, rng, lut, width, channel_mode=False, waterfall=False, detector="peak"):
    """The reply dict (keys as binding.Context.render) plus "M", "counts" and "jstar" [width, n]."""
    fmt = fmt.upper()
    data = np.ascontiguousarray(data, dtype=np.uint8)
    lut = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
    L = len(lut)
    M, counts = subframe_rule(fmt, n, data.size, width)
    if detector != "peak":
        M, counts = 1, [1] * width
    inj = np.stack([np.arange(L) & 255, np.arange(L) >> 8, np.zeros(L, int)], axis=1).astype(np.uint8)
    off = _pixel_offsets(n, width, waterfall)
    held = jstar = gray = db = None
    amps = None
    for j in range(M):
        shift = j * n * SW[fmt]
        shifted = np.concatenate([data[shift:], np.zeros(min(shift, data.size), np.uint8)])
        assert shifted.size == data.size
        r = pyoracle.render(fmt, shifted, n, windowc, block_norm, gain, rng, inj, width, channel_mode, waterfall, planes=True)
        g = r["rgba"][off].astype(np.int64) + 256 * r["rgba"][off + 1].astype(np.int64)      # the plane's colour index per (x, i)
        if j == 0:
            held, db, gray = r["abs2"].copy(), r["db"].copy(), g
            jstar = np.zeros((width, n), np.int64)
            amps = r["gauge_amps"].copy()
            continue
        exists = (np.asarray(counts) > j)[:, None]
        take = exists & ((r["abs2"] > held) | np.isnan(held))
        held = np.where(take, r["abs2"], held)
        db = np.where(take, r["db"], db)
        gray = np.where(take, g, gray)
        jstar = np.where(take, j, jstar)
    out = {"M": M, "counts": counts, "jstar": jstar}
    rgba = np.zeros(4 * width * n, np.uint8)
    for c in range(3):
        rgba[off + c] = lut[gray, c]
    rgba[off + 3] = 255
    out["rgba"] = rgba
    out["c_hist"] = np.bincount(gray.ravel(), minlength=L).astype(np.int64)
    with np.errstate(all="ignore"):
        t = 0.5 + db * -10                                            # worker.js:105-106
        cb = np.where(np.isfinite(t), np.trunc(t), 0.0).astype(np.int64)
        cb = np.where(cb >= 1000, 999, cb)
        out["cB_hist"] = np.bincount(cb[cb >= 0].ravel(), minlength=1000).astype(np.int64)
        fmin = np.fmin(np.fmin.reduce(db, axis=1), 0.0) if width else np.zeros(0)     # worker.js:102-103: a NaN never wins a comparison
        fmax = np.fmax(np.fmax.reduce(db, axis=1), -200.0) if width else np.zeros(0)
        out["dBfs_min"] = float(np.fmin(fmin.min(), 0.0)) if width else 0.0          # worker.js:124-125
        out["dBfs_max"] = float(np.fmax(fmax.max(), -200.0)) if width else -200.0
        out["gauge_mins"] = _clamp_u8(0.5 + (rng + fmin) * 256 / rng)                # worker.js:126-129
        out["gauge_maxs"] = _clamp_u8(0.5 + (rng + fmax) * 256 / rng)
    out["gauge_amps"] = amps if amps is not None else np.zeros(0, np.uint8)
    return out


KEYS = ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps")


def assert_same(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), "%s: %s differs (%d places)" % (what, k, int(np.count_nonzero(got[k] != want[k])))
    assert np.array_equal(np.asarray(got["c_hist"]).astype(np.int64), want["c_hist"]), what + ": c_hist differs"
    assert np.array_equal(np.asarray(got["cB_hist"]).astype(np.int64), want["cB_hist"]), what + ": cB_hist differs"
    assert got["dBfs_min"] == want["dBfs_min"] and got["dBfs_max"] == want["dBfs_max"], \
        "%s: dBfs range %r %r, expected %r %r" % (what, got["dBfs_min"], got["dBfs_max"], want["dBfs_min"], want["dBfs_max"])
