"""The reference of the burst measurements (include/spectroplot_hip.h, "Burst measurements"): burstref's bursts, and per burst
math.fsum of its frames (meanref.exact_sum, on magnitudes) and a plain Python loop for the peak - no integer keys, no cells.  The
series are burstref's planted series with values planted on top in known places; telling() asserts every plant on the EXPECTED arrays
before anything runs on a device.

measure(row, hi, lo)                          [(start, end, energy, peak, peak_at), ...] of one series
expected(series, hi, lo, max_bursts)          (counts, edges, energy, peak, peak_at) as the library replies, energy and peak as uint64 bits
planted_series(seed, count, width, segment)   (series f64 [count, width], hi, lo), read-only and cached
planted_expected(seed, count, width, segment) the uncut reply of that series
cut(reply, max_bursts)                        the reply for a smaller max_bursts out of an uncut one
telling(seed, count, width, segment)          the names of the plants the expected arrays show
must_tell(seed, count, width, segment)        what telling() has to find at that shape
"""
import functools
import math

import numpy as np

import burstref
import meanref

NAN_BITS = 0x7FF8000000000000      # the one NaN an energy is
FILL_BITS = 0xFFFFFFFFFFFFFFFF     # behind the listed bursts
T53 = 2.0 ** 53
T54 = 2.0 ** 54


def bits_of(v):
    return int(np.array([v], np.float64).view(np.uint64)[0])


def measure(row, hi, lo):
    """The bursts of one series with their measurements: the energy is math.fsum of the magnitudes with the rule of the specials, the
    peak the largest magnitude that is no NaN, found with `>` frame by frame so that the earliest of equal maxima stays."""
    row = np.abs(np.asarray(row, np.float64))
    out = []
    for s, e in burstref.scan(row, hi, lo):
        vals = row[s:e].tolist()
        peak, at = None, -1
        for k, v in enumerate(vals):
            if v == v and (peak is None or v > peak):
                peak, at = v, s + k
        out.append((s, e, meanref.exact_sum(vals), peak, at))
    return out


def expected(series, hi, lo, max_bursts):
    series = np.asarray(series, np.float64)
    count = series.shape[0]
    counts = np.zeros(count, np.uint32)
    edges = np.full((count, max_bursts, 2), -1, np.int32)
    energy = np.full((count, max_bursts), FILL_BITS, np.uint64)
    peak = np.full((count, max_bursts), FILL_BITS, np.uint64)
    peak_at = np.full((count, max_bursts), -1, np.int32)
    for b in range(count):
        found = measure(series[b], hi[b], lo[b])
        counts[b] = len(found)
        for i, (s, e, en, pk, at) in enumerate(found[:max_bursts]):
            edges[b, i] = (s, e)
            energy[b, i] = NAN_BITS if en != en else bits_of(en)
            peak[b, i] = bits_of(pk)
            peak_at[b, i] = at
    return counts, edges, energy, peak, peak_at


def cut(reply, max_bursts):
    counts, edges, energy, peak, peak_at = reply
    k = min(max_bursts, edges.shape[1])
    out = [counts.copy(), np.full((edges.shape[0], max_bursts, 2), -1, np.int32), np.full((edges.shape[0], max_bursts), FILL_BITS, np.uint64),
           np.full((edges.shape[0], max_bursts), FILL_BITS, np.uint64), np.full((edges.shape[0], max_bursts), -1, np.int32)]
    for dst, src in zip(out[1:], (edges, energy, peak, peak_at)):
        dst[:, :k] = src[:, :k]
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- the plants
# name -> (band, [(frame, value), ...], the burst's start, what the expected burst must show).  Band 0 has HI = 8, LO = 2 and is OFF
# between burstref's own plants (frames 0 .. 9, S - 1, S, 2 S, 3 S - 1, 4 S - 3 .. 5 S + 2); band 4 has lo < 0 and is ONE burst from
# frame 3 on; band 5 has lo = 1e-320, hi = 1: 2^-1022 and 1e-300 HOLD there, 0.0 resets.
def _plants(S):
    p = {
        # a tie, two frames: 2^54 + 2 lies halfway between 2^54 and 2^54 + 4, the even one is 2^54; the maximum is the FIRST frame
        "tie_down_peak_first": (0, [(20, T54), (21, 2.0), (22, 0.0)], 20, dict(end=22, energy=T54, peak=T54, at=20)),
        # ... and 2^54 + 6 halfway between 2^54 + 4 and 2^54 + 8: the even one is 2^54 + 8
        "tie_up": (0, [(24, T54 + 4), (25, 2.0), (26, 0.0)], 24, dict(end=26, energy=T54 + 8, peak=T54 + 4, at=24)),
        # a finite sum beyond DBL_MAX
        "overflow": (0, [(28, 1.5e308), (29, 1.5e308), (30, 0.0)], 28, dict(end=30, energy=math.inf, peak=1.5e308, at=28)),
        # the maximum on the burst's LAST frame
        "peak_last": (0, [(34, 9.0), (35, 10.0), (36, 100.0), (37, 0.0)], 34, dict(end=37, energy=119.0, peak=100.0, at=36)),
        # 1e300 beside 1e-300, equal maxima: the earliest
        "huge_beside_tiny": (5, [(29, 0.0), (30, 1e300), (31, 1e-300), (32, 1e300), (33, 0.0)], 30,
                             dict(end=33, energy=2e300, peak=1e300, at=30)),
        # three addends a left-to-right float sum gets wrong: 2^53 + 1 + 1 (+ 2^-1022, sticky below)
        "naive_fails": (5, [(35, 0.0), (36, T53), (37, 1.0), (38, 1.0), (39, 2.0 ** -1022), (40, 0.0)], 36,
                        dict(end=40, energy=T53 + 2, peak=T53, at=36, naive_differs=True)),
        # the whole exponent range in ONE long burst: band 4 from frame 3 to the width
        "exponent_spread": (4, [(10, 2.0 ** -1074), (11, 2.0 ** -1022), (12, 1.0), (13, T53), (14, T53 + 2)], 3, dict(peak=T53 + 2, at=14)),
    }
    if S >= 64:
        # burstref's burst across three segments [4 S - 3, 5 S + 2): equal maxima in its first and its third segment
        p["equal_maxima_first_and_third_segment"] = (0, [(4 * S - 2, 77.0), (5 * S + 1, 77.0)], 4 * S - 3, dict(end=5 * S + 2, peak=77.0, at=4 * S - 2))
        # burstref's burst [2 S, 3 S - 1): the maximum on its last frame; and the one-frame burst [S - 1, S) on the last frame of a segment
        p["peak_before_the_fall"] = (0, [(3 * S - 2, 55.0)], 2 * S, dict(end=3 * S - 1, peak=55.0, at=3 * S - 2))
        p["peak_last_of_segment"] = (0, [], S - 1, dict(end=S, energy=9.0, peak=9.0, at=S - 1))
    return p


def _fits(plant, count, width):
    band, frames, start, _ = plant
    last = max([x for x, _ in frames] + [start])
    return band < count and last + 1 < width   # (one frame of room behind it: burstref's open burst on the last frame stays)


@functools.lru_cache(maxsize=None)
def _planted(seed, count, width, segment):
    series, hi, lo = burstref.planted_series(seed, count, width, segment)
    series = series.copy()
    for plant in _plants(segment).values():
        if _fits(plant, count, width):
            for x, v in plant[1]:
                series[plant[0], x] = v
    series.setflags(write=False)
    return series, hi, lo


def planted_series(seed, count, width, segment):
    """(series f64 [count, width], hi, lo), read-only and cached: burstref.planted_series with this module's plants on top."""
    return _planted(int(seed), int(count), int(width), int(segment))


@functools.lru_cache(maxsize=None)
def planted_expected(seed, count, width, segment):
    """The uncut reply of planted_series of that shape, max_bursts = width // 2 + 1; read-only."""
    series, hi, lo = planted_series(seed, count, width, segment)
    reply = expected(series, hi, lo, width // 2 + 1)
    for a in reply:
        a.setflags(write=False)
    return reply


def naive_sum(vals):
    s = 0.0
    with np.errstate(all="ignore"):
        for v in vals:
            s = float(np.float64(s) + np.float64(v))
    return s


def must_tell(seed, count, width, segment):
    need = {name for name, plant in _plants(segment).items() if _fits(plant, count, width)}
    if width > 5:
        need.add("nan_inside_a_burst")       # burstref's frame 4
    if width > 9:
        need.add("inf_frame")                # burstref's frame 8
    if "open_at_end" in burstref.must_tell(seed, count, width, segment) or (count > 4 and width > 3):   # (band 4 never resets)
        need.add("open_at_width")
    if count > 1 and width >= 2:
        need.add("alternating")
    if count > 2 and width >= 1:
        need.add("never_bursts")
    if width > 5 * segment + 2 and segment >= 64:
        need.add("across_three_segments")
    return need


def telling(seed, count, width, segment):
    """The names of the plants that the EXPECTED arrays of planted_series(seed, count, width, segment) show, each asserted in full."""
    series, hi, lo = planted_series(seed, count, width, segment)
    counts, edges, energy, peak, peak_at = planted_expected(seed, count, width, segment)
    seen = set()

    def burst_at(b, start):
        hit = np.flatnonzero(edges[b, :counts[b], 0] == start)
        assert hit.size == 1, (b, start)
        return int(hit[0])

    for name, plant in _plants(segment).items():
        if not _fits(plant, count, width):
            continue
        b, _, start, want = plant
        i = burst_at(b, start)
        s, e = edges[b, i]
        if "end" in want:
            assert e == want["end"], name
        if "energy" in want:
            assert energy[b, i] == bits_of(want["energy"]), name
        assert peak[b, i] == bits_of(want["peak"]) and peak_at[b, i] == want["at"], name
        if want.get("naive_differs"):
            assert bits_of(naive_sum(series[b, s:e])) != energy[b, i], name
        seen.add(name)
    if "exponent_spread" in seen:   # (a long burst of hundreds of addends: the float sum is off as well, wherever it has the room)
        i = burst_at(4, 3)
        assert edges[4, i, 1] == width
    for b in range(count):
        for i in range(int(counts[b])):
            s, e = edges[b, i]
            row = series[b, s:e]
            nan = row != row
            assert not nan[0]
            if nan.any():
                assert energy[b, i] == NAN_BITS and peak[b, i] == bits_of(np.nanmax(row)) and series[b, peak_at[b, i]] == np.nanmax(row)
                seen.add("nan_inside_a_burst")
            elif (row == math.inf).any():
                assert energy[b, i] == peak[b, i] == bits_of(math.inf) and peak_at[b, i] == s + int(np.argmax(row == math.inf))
                seen.add("inf_frame")
            if e == width:
                seen.add("open_at_width")
            if e < width and e // segment >= s // segment + 2:
                seen.add("across_three_segments")
        if width >= 2 and counts[b] == width // 2 and (edges[b, :counts[b], 1] - edges[b, :counts[b], 0] == 1).all():
            k = int(counts[b])
            assert (energy[b, :k] == series[b, edges[b, :k, 0]].view(np.uint64)).all() and (peak[b, :k] == energy[b, :k]).all()
            assert (peak_at[b, :k] == edges[b, :k, 0]).all()
            seen.add("alternating")
        if width and counts[b] == 0:
            assert (energy[b] == FILL_BITS).all() and (peak_at[b] == -1).all()
            seen.add("never_bursts")
    return seen
