"""Edge-straddle harness: captures that put |X|^2 onto both sides of every step of every output scale, a few ulps apart, and the
parameter sets / shapes the GPU comparisons run them at (tests/test_edges_gpu.py) and the CPU self-check verifies (tests/test_edges_cpu.py).

Built on the oracle alone (oracle/pyoracle.py): nothing here reads the product's threshold tables, so an expected value never depends
on the code under test.  The construction: a CF64 frame whose only non-zero sample is (x, 0) at index 0 under a taper with
w[0] == 1.0 (any finite values elsewhere) has abs2 == x*x, bit for bit, in every bin in I/Q mode; in L/R mode x*x in the bins
i < n/2 and exactly 0 in the others.  The same holds for a sample at index n/2 with abs2 == (w[n/2] * x)^2 (the non-zero value only
ever is the untwiddled operand of a butterfly).  tests/test_edges_cpu.py checks both statements with the oracle's planes.
Test infrastructure, not a test.
"""
import collections
import functools
import struct

import numpy as np

from oracle import pyoracle

FMT = "CF64"
SEARCH_LO, SEARCH_HI = 1e-200, 1e200

ParamSet = collections.namedtuple("ParamSet", "name gain rng lut_len block_norm")

# --- the parameter sets of the n = 64 sweep: all inside plan_frames_capable's domain (the GPU test asserts kernel_name() == "frames") ---
DEFAULT = ParamSet("default", 6.0, 30.0, 256, 1.0 / 64)
# gray_b = 1.505 * lut_len / range = 1927 of the 2000 allowed, the largest edge at 2^93, |a| = 1.7e5, l_max = 94: the widest margin
# (0.045 steps) of the list, and the colour edges (2^89) lie inside the level scale's clamp range, where the f32 decision is taken
STRAINED = ParamSet("steep_high_edges", 6.0, 0.2, 256, 1e-14)
SWEEP = [
    DEFAULT,
    ParamSet("steep_edges_near_1", 0.0, 0.25, 256, 1.0),                       # gray_b = 1541, colour edges in [2^-0.17, 1]
    STRAINED,
    ParamSet("steep_low_edges", 95.0, 0.25, 256, 31622.776601683792),          # smallest edge 2^-96, colour edges at 2^-93
    ParamSet("gain_plus_250", 250.0, 30.0, 256, 3.16e-15),                     # colour edges 2^-90 .. 2^-70, level edges 2^30 .. 2^96
    ParamSet("gain_minus_180", -180.0, 30.0, 256, 1e4),                        # colour edges 2^73 .. 2^93, level edges 2^-93 .. 2^-27
    ParamSet("lut_2", 6.0, 30.0, 2, 1.0 / 64),
    ParamSet("lut_3", 6.0, 30.0, 3, 1.0 / 64),
    ParamSet("lut_17", 6.0, 30.0, 17, 1.0 / 64),
    ParamSet("lut_255", 6.0, 30.0, 255, 1.0 / 64),
    ParamSet("range_300", -50.0, 300.0, 256, 1e-10),                           # colour steps 1.17 dB wide, edges 2^-98.5 .. 2^99.3
    ParamSet("range_300_lut_17", -50.0, 300.0, 17, 1e-10),
]
# ... and two just outside it: the plan must choose the scratch kernel, and the reply must still be exact
OUTSIDE = [
    ParamSet("gray_b_2028", 0.0, 0.19, 256, 1.0),                              # 1.505 * 256 / 0.19 > 2000
    ParamSet("edge_at_2_106", 6.0, 30.0, 256, 1e-16),                          # level edges up to 2^106 > 2^100
]
OFFSETS5 = (-2, -1, 0, 1, 2)
OFFSETS3 = (-1, 0, 1)

# --- every epilogue instantiation: (set, n, L/R split, waterfall, flat taper, offsets).  The strained set runs under the bumpy taper.
EPILOGUE = [(s, n, ch, ch != (n in (256, 1024, 4096)), s is DEFAULT, OFFSETS5 if n <= 1024 else OFFSETS3)
            for s in (DEFAULT, STRAINED) for n in (128, 256, 512, 1024, 2048, 4096, 8192) for ch in (False, True)]
GAUGE_NS = (64, 1024, 2048)           # in-kernel side outputs: one shape per synchronisation regime
GAUGE_SETS = (DEFAULT, SWEEP[10])    # range 300: gauge_maxs meets its -200 dB floor inside the byte scale
BATCH_NS = (64, 128, 256, 512)        # the documented domain of k_frames_batch
BATCH_SETS = (DEFAULT, STRAINED)
PEAK_M = 3
PEAK_CASES = [(s, n, ch) for s in (DEFAULT, STRAINED) for n in (64, 256, 1024) for ch in (False, True)]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def step_points(f, lo=SEARCH_LO, hi=SEARCH_HI):
    """The smallest doubles in (lo, hi] at which f changes its value, ascending, by bisection over bit patterns (f is a monotone
    step function of a positive double)."""
    out = []
    a, b = _bits(lo), _bits(hi)
    stack = [(a, f(lo), b, f(hi))]
    while stack:
        a, fa, b, fb = stack.pop()
        if fa == fb:
            continue
        if b - a == 1:
            out.append(_from_bits(b))
            continue
        m = a + (b - a) // 2
        fm = f(_from_bits(m))
        stack.append((m, fm, b, fb))
        stack.append((a, fa, m, fm))       # popped first: ascending order
    return np.array(out, dtype=np.float64)


def _clamp_u8(v):
    """A store into a Uint8ClampedArray (oracle/sp_oracle.c js_clamp_u8): NaN and negatives 0, round half to even, 255 at most."""
    if not v > 0:
        return 0
    if v >= 255:
        return 255
    return int(round(v))


class Scales:
    """The reference's per-pixel and per-column arithmetic as functions of abs2, in its operation order (oracle/sp_oracle.c:303-358),
    with the oracle's own log10."""

    def __init__(self, gain, rng, lut_len, block_norm):
        self.log10 = pyoracle.lib().spo_log10
        self.gain, self.rng = float(gain), float(rng)
        self.bndb = 10 * self.log10(block_norm)
        self.cmax = float(lut_len - 1)
        self.color_norm = float(lut_len) / -self.rng

    def dbfs(self, a2):
        return 5 * self.log10(a2) + self.bndb + self.gain

    def gray(self, a2):
        u = self.cmax - self.dbfs(a2) * self.color_norm
        return int(0.5 + (0 if u < 0 else self.cmax if u > self.cmax else u))

    def cbin(self, a2):
        """the key of cB_hist; -1: dropped (a negative key)"""
        v = 0.5 + (self.dbfs(a2) - self.gain) * -10
        c = int(v)                                   # ToInt32 of a finite value of this size: truncation
        return 999 if c >= 1000 else c if c >= 0 else -1

    def _gauge(self, v):
        return _clamp_u8(0.5 + (self.rng + v) * 256 / self.rng)

    def gauge_min(self, a2):
        d = self.dbfs(a2) - self.gain
        return self._gauge(d if d < 0.0 else 0.0)

    def gauge_max(self, a2):
        d = self.dbfs(a2) - self.gain
        return self._gauge(d if d > -200.0 else -200.0)

    def gauge_amp(self, raw2):
        """of the raw centre sample: ci^2 + cq^2, no taper, no block_norm"""
        return self._gauge(5 * self.log10(raw2) + self.gain)


@functools.lru_cache(maxsize=None)
def index_edges(gain, rng, lut_len, block_norm):
    """(colour edges, centi-bel edges): the doubles at which the oracle's colour index / cB_hist key change."""
    s = Scales(gain, rng, lut_len, block_norm)
    return step_points(s.gray), step_points(s.cbin)


@functools.lru_cache(maxsize=None)
def gauge_edges(gain, rng, block_norm):
    """{"mins", "maxs", "amps"}: the doubles at which the byte js_clamp_u8(0.5 + (range + v) * 256 / range) changes, as a function of
    abs2 for v = min(d, 0) and v = max(d, -200), and of the raw centre sample's square for gauge_amps: the points where one ulp of a
    log10 result moves a byte."""
    s = Scales(gain, rng, 2, block_norm)
    return {"mins": step_points(s.gauge_min), "maxs": step_points(s.gauge_max), "amps": step_points(s.gauge_amp)}


def all_index_edges(ps):
    g, c = index_edges(ps.gain, ps.rng, ps.lut_len, ps.block_norm)
    return np.concatenate([g, c])


def straddle_values(edges, offsets):
    """x[e, k] = sqrt(edges[e]) with its bit pattern moved by offsets[k]."""
    r = np.sqrt(np.asarray(edges, dtype=np.float64))
    return (r.view(np.int64)[:, None] + np.asarray(offsets, dtype=np.int64)[None, :]).view(np.float64)


def straddle_capture(edges, n, offsets, index=0):
    """One CF64 frame per (edge, offset), its only non-zero sample (x, 0) at `index`.  Returns (bytes, width, x[edge, offset]);
    stride == n exactly, so frame f is the capture's samples [f * n, (f + 1) * n)."""
    xs = straddle_values(edges, offsets)
    cap = np.zeros((xs.size, n, 2), dtype=np.float64)
    cap[:, index, 0] = xs.reshape(-1)
    return cap.reshape(-1).view(np.uint8), xs.size, xs


def straddles(xs, edges, scale=1.0):
    """Condition (ii): for every edge, the squares of its x values lie on both sides, min < edge <= max.  Boolean per edge."""
    sq = (scale * xs) * (scale * xs)
    e = np.asarray(edges, dtype=np.float64)
    return (sq.min(axis=1) < e) & (e <= sq.max(axis=1))


def taper(n, flat):
    """w[0] == 1; flat: all ones, else arbitrary finite values elsewhere (both signs, four decades)."""
    if flat:
        return np.ones(n, dtype=np.float64)
    r = np.random.RandomState(n)
    w = (0.25 + 1.5 * r.random_sample(n)) * np.where(r.random_sample(n) < 0.3, -1.0, 1.0) * 10.0 ** r.randint(-2, 3, n)
    w[0] = 1.0
    return w


def lut(lut_len):
    """Red = colour index (lut_len <= 256): the number of distinct reds in an image is the number of colour indices that occur."""
    i = np.arange(lut_len)
    return np.stack([i & 255, (255 - i) & 255, (i * 7) & 255], axis=1).astype(np.uint8)


def peak_capture(edges, n, offsets, m=PEAK_M, variants="abc"):
    """A capture of stride exactly m * n (samples = n + (width - 1) * m * n): column c holds m sub-frames.  One column per
    (edge, offset); it carries the straddling x in sub-frame j and in its other sub-frames (a) silence, (b) x / 2 or (c) the double one
    bit below x - so the hold, not the first or the last sub-frame, decides on which side of the edge the column lands.  The
    (variant, j) pairs rotate over the columns, so every pair meets values on both sides of edges all along the scales.
    The last column of a peak request has one sub-frame only; a copy of column 0's value in sub-frame 0 is appended there.
    Returns (bytes, width, x[column], [(variant, j)] per column but the last)."""
    xs = straddle_values(edges, offsets).reshape(-1)
    pairs = [(v, j) for v in variants for j in range(m)]
    per = xs.size
    width = per + 1
    frames = np.zeros((per * m + 1, n, 2), dtype=np.float64)
    below = (xs.view(np.int64) - 1).view(np.float64)
    other = {"a": np.zeros(per), "b": xs / 2, "c": below}
    which = np.arange(per) % len(pairs)
    for k, (v, j) in enumerate(pairs):
        c = np.nonzero(which == k)[0]
        for s in range(m):
            frames[c * m + s, 0, 0] = xs[c] if s == j else other[v][c]
    frames[per * m, 0, 0] = xs[0]
    return frames.reshape(-1).view(np.uint8), width, np.append(xs, xs[0]), [pairs[k] for k in which]


def peak_edge_subset(ps, n):
    """All index edges up to n = 256, every fourth at n = 1024: the oracle's work per case stays below two million bins per sub-frame."""
    e = all_index_edges(ps)
    step = max(n // 256, 1)
    return e[step // 2::step]


def log10_probe_values(count=200):
    """x values for one-frame requests with block_norm = 1, gain = 0, where dBfs_min / dBfs_max == 5 * log10(x * x): the square roots of
    gauge edges (log10 results next to a rounding boundary of the byte) and seeded values over 2^-60 .. 2^60."""
    e = gauge_edges(0.0, 60.0, 1.0)["mins"]
    pick = e[:: max(len(e) // (count // 2), 1)][: count // 2]
    r = np.random.RandomState(20261016)
    spread = np.ldexp(1.0 + r.random_sample(count - len(pick)), r.randint(-60, 61, count - len(pick)))
    return np.concatenate([np.sqrt(pick), spread])


def chunks(width, n, limit=1 << 22):
    """Frame ranges [a, b) of at most `limit` bins for walking a large capture through the oracle piece by piece (stride == n)."""
    step = max(limit // n, 1)
    return [(a, min(a + step, width)) for a in range(0, width, step)]
