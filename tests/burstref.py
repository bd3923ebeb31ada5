"""The reference of the burst lists (include/spectroplot_hip.h, "Burst lists"): a plain loop per band with `s >= hi` and `s < lo` as
floating-point compares - not the library's integer keys - and series with every case that matters planted in known places.

scan(row, hi, lo)                      the bursts [(start, end), ...] of one series
expected(series, hi, lo, max_bursts)   (counts uint32 [count], edges int32 [count, max_bursts, 2]) as the library replies
planted_series(seed, count, width, segment)   (series f64 [count, width], hi f64 [count], lo f64 [count])
telling(series, hi, lo, segment)       which of the planted conditions the expected bursts show
must_tell(seed, count, width, segment) which of them a series of that shape has room for
"""
import functools
import math

import numpy as np

HI, LO = 8.0, 2.0                 # band 0's thresholds, and most bands'
DEN_LO = 1e-320                   # a denormal `lo`
ROLES = ("planted", "alternating", "none", "equal", "negative", "denormal")   # of band b: ROLES[b % 6]


def scan(row, hi, lo):
    """The bursts of one series, [(start, end), ...]: the state machine of the header, frame by frame."""
    hi, lo = float(hi), float(lo)
    out, on, start = [], False, 0
    for x, s in enumerate(np.asarray(row, np.float64).tolist()):
        if s >= hi:              # SET (False for a NaN)
            if not on:
                on, start = True, x
        elif s < lo:             # RESET (False for a NaN)
            if on:
                on = False
                out.append((start, x))
    if on:
        out.append((start, len(row)))
    return out


def expected(series, hi, lo, max_bursts):
    series = np.asarray(series, np.float64)
    count = series.shape[0]
    counts = np.zeros(count, np.uint32)
    edges = np.full((count, max_bursts, 2), -1, np.int32)
    for b in range(count):
        bursts = scan(series[b], hi[b], lo[b])
        counts[b] = len(bursts)
        k = min(len(bursts), max_bursts)
        if k:
            edges[b, :k] = np.array(bursts[:k], np.int32)
    return counts, edges


def cut(counts, edges, max_bursts):
    """The reply for another max_bursts out of an uncut one: the first max_bursts bursts of every band, -1 behind them."""
    out = np.full((edges.shape[0], max_bursts, 2), -1, np.int32)
    k = min(max_bursts, edges.shape[1])
    out[:, :k] = edges[:, :k]
    return counts.copy(), out


def thresholds(count):
    hi, lo = np.full(count, HI), np.full(count, LO)
    for b in range(count):
        role = ROLES[b % 6]
        if role == "equal":
            lo[b] = hi[b] = 5.0
        elif role == "negative":
            lo[b] = -1.0
        elif role == "denormal":
            lo[b], hi[b] = DEN_LO, 1.0
    return hi, lo


def _plants(seed, width, S):
    """Band 0's planted frames, (x, value) in time order; a frame at or past `width` does not exist."""
    below = lambda v: math.nextafter(v, 0.0)   # noqa: E731
    p = [(0, math.nan if seed % 2 == 0 else HI),           # NaN as the very first frame / a burst from frame 0, by the seed
         (1, HI),                                          # equal to hi: SET
         (2, below(HI)), (3, LO), (4, math.nan),           # one ulp below hi, equal to lo, a NaN while ON: all HOLD
         (5, below(LO)),                                   # one ulp below lo: RESET
         (6, math.nan), (7, below(HI)),                    # a NaN while OFF, one ulp below hi while OFF: HOLD
         (8, math.inf), (9, 0.0)]                          # +inf: SET
    if S >= 16:
        p += [(S - 1, 9.0), (S, 0.0),                      # a rise on the last frame of a segment, a fall on the first of the next
              (2 * S, 9.0), (3 * S - 1, 0.0),              # a rise on the first frame of a segment, a fall on the last
              (4 * S - 3, 9.0), (5 * S + 2, 0.0)]          # one burst across three segments, the middle one all HOLD
    p = [(x, v) for x, v in p if x < width]
    if width >= 12 and all(x != width - 1 for x, _ in p):
        p.append((width - 1, 9.0))                         # a burst open at the end
    return p


@functools.lru_cache(maxsize=None)
def _planted(seed, count, width, segment):
    rng = np.random.default_rng(seed * 7919 + count * 131 + width)
    hi, lo = thresholds(count)
    series = np.empty((count, width))
    for b in range(count):
        role, row = ROLES[b % 6], series[b]
        row[:] = rng.uniform(3.0, 7.0, width)              # HOLD for HI / LO
        if role == "planted":
            if b:                                          # band 0 holds the plants alone; its likes further up get random events too
                ev = rng.random(width) < 0.2
                row[ev] = rng.choice([0.0, 1.0, 9.0, 30.0], int(ev.sum()))
                nan = rng.random(width) < 0.02
                row[nan] = math.nan
            for x, v in _plants(seed, width, segment):
                row[x] = v
        elif role == "alternating":                        # RESET, SET, RESET, ...: width // 2 bursts of one frame
            row[0::2], row[1::2] = 1.0, 9.0
        elif role == "none":
            row[rng.random(width) < 0.3] = 0.5             # RESETs and HOLDs only
        elif role == "equal":                              # lo == hi == 5: every frame is a SET or a RESET, or a NaN
            row[rng.random(width) < 0.05] = math.nan
            row[rng.random(width) < 0.05] = 5.0
        elif role == "negative":                           # lo < 0: the first SET is never undone
            row[rng.random(width) < 0.1] = 0.0
            if width > 3:
                row[3] = 9.0
        elif role == "denormal":                           # lo = 1e-320, hi = 1: denormals around lo
            row[:] = rng.choice([0.5, DEN_LO, 2e-320, 5e-321, 5e-324, 0.0, 1.5], width, p=[0.5, 0.1, 0.1, 0.1, 0.05, 0.05, 0.1])
    series.setflags(write=False)
    hi.setflags(write=False)
    lo.setflags(write=False)
    return series, hi, lo


def planted_series(seed, count, width, segment):
    """(series f64 [count, width], hi, lo), read-only and cached: band b plays ROLES[b % 6]."""
    return _planted(int(seed), int(count), int(width), int(segment))


@functools.lru_cache(maxsize=None)
def planted_expected(seed, count, width, segment):
    """The uncut reply of planted_series of that shape: (counts, edges [count, width // 2 + 1, 2])."""
    series, hi, lo = planted_series(seed, count, width, segment)
    counts, edges = expected(series, hi, lo, width // 2 + 1)
    counts.setflags(write=False)
    edges.setflags(write=False)
    return counts, edges


def telling(series, hi, lo, segment):
    """The names of the planted conditions that the EXPECTED bursts of this series show."""
    series = np.asarray(series, np.float64)
    count, width = series.shape
    S, seen = segment, set()
    below = lambda v: math.nextafter(v, 0.0)   # noqa: E731
    for b in range(count):
        row, h, l = series[b], float(hi[b]), float(lo[b])
        bursts = scan(row, h, l)
        on = np.zeros(width + 1, bool)
        for s, e in bursts:
            on[s:e] = True
        starts, ends = {s for s, _ in bursts}, {e for _, e in bursts if e < width}
        st, en, onx = np.zeros(width, bool), np.zeros(width, bool), on[:width]
        st[sorted(starts)] = True
        en[sorted(ends)] = True
        nan = row != row
        den = 0 < l < 2.3e-308
        for name, where in (("equal_hi_sets", (row == h) & st), ("equal_lo_holds", (row == l) & onx & ~st),
                            ("below_lo_resets", (row == below(l)) & en if l > 0 else nan[:0]), ("below_hi_holds", (row == below(h)) & ~onx),
                            ("nan_first", nan[:1] & ~onx[:1]), ("nan_on", nan & onx), ("nan_off", nan[1:] & ~onx[1:]),
                            ("inf_sets", (row == math.inf) & st), ("denormal_resets", (row > 0) & (row < l) & en if den else nan[:0]),
                            ("denormal_equal_lo_holds", (row == l) & onx if den else nan[:0])):
            if where.any():
                seen.add(name)
        for s, e in bursts:
            if s == 0:
                seen.add("from_frame_0")
            if e == width:
                seen.add("open_at_end")
            if s > 0 and s % S == 0:
                seen.add("rise_first_of_segment")
            if s % S == S - 1:
                seen.add("rise_last_of_segment")
            if e < width and e % S == 0:
                seen.add("fall_first_of_segment")
            if e < width and e % S == S - 1:
                seen.add("fall_last_of_segment")
            if e < width and e // S >= s // S + 2:
                mid = row[(s // S + 1) * S:(s // S + 2) * S]
                if ((mid < h) & (mid >= l)).all():
                    seen.add("across_three_segments")
        if width >= 2 and len(bursts) == width // 2 and all(e - s == 1 for s, e in bursts):
            seen.add("alternating")
        if width and not bursts:
            seen.add("no_burst")
        if l == h and bursts:
            seen.add("lo_equals_hi")
        if l < 0 and len(bursts) == 1 and bursts[0][1] == width:
            seen.add("negative_lo_never_resets")
    return seen


def must_tell(seed, count, width, segment):
    """What telling() has to find for planted_series(seed, count, width, segment): every condition the shape has room for."""
    S, w, need = segment, width, set()
    if seed % 2 == 0:
        if w >= 1:
            need.add("nan_first")
    elif w >= 1:
        need.add("from_frame_0")
    for x, name in ((1 if seed % 2 == 0 else 0, "equal_hi_sets"), (3, "equal_lo_holds"), (4, "nan_on"), (5, "below_lo_resets"), (6, "nan_off"),
                    (7, "below_hi_holds"), (8, "inf_sets")):
        if w > x:
            need.add(name)
    if w >= 1 and dict(_plants(seed, w, S)).get(w - 1, 0.0) >= HI:   # (the last frame is a planted SET)
        need.add("open_at_end")
    if S >= 16:
        for x, name in ((S - 1, "rise_last_of_segment"), (S, "fall_first_of_segment"), (2 * S, "rise_first_of_segment"),
                        (3 * S - 1, "fall_last_of_segment"), (5 * S + 2, "across_three_segments")):
            if w > x:
                need.add(name)
    if count > 1 and w >= 2:
        need.add("alternating")
    if count > 2 and w >= 1:
        need.add("no_burst")
    if count > 3 and w >= 64:
        need.add("lo_equals_hi")
    if count > 4 and w > 3:
        need.add("negative_lo_never_resets")
    if count > 5 and w >= 257:
        need |= {"denormal_resets", "denormal_equal_lo_holds"}
    return need
