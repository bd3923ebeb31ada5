"""The edge-straddle harness (tests/edgeref.py) checked with the oracle alone, so that a pass of tests/test_edges_gpu.py means something:
for every parameter set and shape the GPU comparisons use (the lists are edgeref's, shared by both modules)
  (i)   the oracle's planes show abs2 == x*x (or exactly 0 in the upper half of an L/R frame) in every bin of every frame,
  (ii)  every edge's frames hold values on both sides of it, min(x*x) < edge <= max(x*x) - no exceptions,
  (iii) the expected number of edges is found: lut_len - 1 colour edges, 1000 centi-bel edges, 255 per gauge,
  (iv)  neighbouring offsets really give both output values in the oracle's reply for at least 95 % of the colour edges."""
import numpy as np
import pytest

import edgeref
import peakref
from oracle import pyoracle

ALL_SETS = edgeref.SWEEP + edgeref.OUTSIDE


def _ids(ps):
    return ps.name


def _planes_ok(data, width, n, win, ch, want_sq):
    """abs2 of every bin of every frame against want_sq[frame], walked in pieces (stride == n: frames are independent)."""
    frame_bytes = n * 16
    for a, b in edgeref.chunks(width, n):
        r = pyoracle.render(edgeref.FMT, data[a * frame_bytes:b * frame_bytes], n, win, 1.0, 0.0, 30.0, edgeref.lut(2), b - a, ch, False,
                            planes=True)
        a2 = r["abs2"]
        top = n // 2 if ch else n
        if not np.array_equal(a2[:, :top], np.broadcast_to(want_sq[a:b, None], (b - a, top))):
            return False
        if ch and not np.array_equal(a2[:, top:], np.zeros((b - a, n - top))):
            return False
    return True


@pytest.mark.parametrize("ps", ALL_SETS, ids=_ids)
def test_expected_number_of_edges(ps):
    g, c = edgeref.index_edges(ps.gain, ps.rng, ps.lut_len, ps.block_norm)
    assert len(g) == ps.lut_len - 1 and len(c) == 1000
    assert (np.diff(g) > 0).all() and (np.diff(c) > 0).all()
    s = edgeref.Scales(ps.gain, ps.rng, ps.lut_len, ps.block_norm)
    for e in list(g[:: max(len(g) // 7, 1)]) + [g[0], g[-1]]:                  # an edge is the first double of the upper value
        below = float(np.nextafter(e, 0.0))
        assert s.gray(below) + 1 == s.gray(float(e))
    for e in list(c[::97]) + [c[0], c[-1]]:
        below = float(np.nextafter(e, 0.0))
        assert s.cbin(below) - 1 == s.cbin(float(e))


@pytest.mark.parametrize("ps", list(edgeref.GAUGE_SETS), ids=_ids)
def test_expected_number_of_gauge_edges(ps):
    g = edgeref.gauge_edges(ps.gain, ps.rng, ps.block_norm)
    assert len(g["mins"]) == 255 and len(g["amps"]) == 255
    # gauge_maxs starts from -200 dB: a range above 200 dB never shows the bytes below that value's
    lowest = edgeref.Scales(ps.gain, ps.rng, 2, ps.block_norm).gauge_max(edgeref.SEARCH_LO)
    assert len(g["maxs"]) == 255 - lowest and (lowest > 0) == (ps.rng > 200)


@pytest.mark.parametrize("ps", ALL_SETS, ids=_ids)
def test_every_index_edge_has_values_on_both_sides(ps):
    e = edgeref.all_index_edges(ps)
    used = {edgeref.OFFSETS5} | {off for s, _, _, _, _, off in edgeref.EPILOGUE if s is ps}
    for off in used:
        assert edgeref.straddles(edgeref.straddle_values(e, off), e).all(), off


@pytest.mark.parametrize("ps", list(edgeref.GAUGE_SETS), ids=_ids)
def test_every_gauge_edge_has_values_on_both_sides(ps):
    for k, e in edgeref.gauge_edges(ps.gain, ps.rng, ps.block_norm).items():
        assert edgeref.straddles(edgeref.straddle_values(e, edgeref.OFFSETS5), e).all(), k


@pytest.mark.parametrize("ps", ALL_SETS, ids=_ids)
def test_sweep_frames_carry_the_square_in_every_bin_and_show_both_colours(ps):
    n = 64
    e = edgeref.all_index_edges(ps)
    data, width, xs = edgeref.straddle_capture(e, n, edgeref.OFFSETS5)
    assert width == len(e) * 5 and data.size == width * n * 16
    flat = xs.reshape(-1)
    assert _planes_ok(data, width, n, edgeref.taper(n, True), False, flat * flat)
    want = pyoracle.render(edgeref.FMT, data, n, edgeref.taper(n, True), ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), width)
    red = want["rgba"].reshape(n, width, 4)[0, :, 0].reshape(len(e), 5)[:ps.lut_len - 1]       # the colour edges' frames
    both = sum(1 for g in range(ps.lut_len - 1) if {g, g + 1} <= set(red[g].tolist()))
    assert both >= 0.95 * (ps.lut_len - 1), (both, ps.lut_len - 1)
    if ps is edgeref.DEFAULT:
        assert len(np.unique(want["rgba"].reshape(-1, 4)[:, 0])) > 250
    # ... and both keys of every centi-bel edge are counted
    assert np.count_nonzero(want["cB_hist"]) == 1000


@pytest.mark.parametrize("case", edgeref.EPILOGUE, ids=lambda c: "%s_n%d_%s" % (c[0].name, c[1], "lr" if c[2] else "iq"))
def test_epilogue_frames_carry_the_square_in_every_bin(case):
    ps, n, ch, wf, flat, off = case
    data, width, xs = edgeref.straddle_capture(edgeref.all_index_edges(ps), n, off)
    sq = xs.reshape(-1) * xs.reshape(-1)
    assert _planes_ok(data, width, n, edgeref.taper(n, flat), ch, sq)


def test_the_bumpy_taper_is_not_flat_and_finite():
    for n in (64, 8192):
        w = edgeref.taper(n, False)
        assert w[0] == 1.0 and np.isfinite(w).all() and (w < 0).any() and np.ptp(np.abs(w)) > 100 and (w != 0).all()


@pytest.mark.parametrize("n", edgeref.GAUGE_NS)
@pytest.mark.parametrize("ps", list(edgeref.GAUGE_SETS), ids=_ids)
def test_gauge_frames(ps, n):
    """The min / max gauge frames (sample at index 0) and the amp frames (sample at index n/2), under a taper that is 1 at index 0 only: abs2 in
    every bin, and every byte value of each gauge occurs in the oracle's reply."""
    g = edgeref.gauge_edges(ps.gain, ps.rng, ps.block_norm)
    e0 = np.concatenate([g["mins"], g["maxs"]])
    data, width, xs = edgeref.straddle_capture(e0, n, edgeref.OFFSETS5)
    flat = xs.reshape(-1)
    w = edgeref.taper(n, False)
    assert _planes_ok(data, width, n, w, False, flat * flat)
    want = pyoracle.render(edgeref.FMT, data, n, w, ps.block_norm, ps.gain, ps.rng, edgeref.lut(256), width)
    assert len(np.unique(want["gauge_mins"])) == 256 and len(np.unique(want["gauge_maxs"])) == len(g["maxs"]) + 1
    data, width, xs = edgeref.straddle_capture(g["amps"], n, edgeref.OFFSETS5, index=n // 2)
    wx = w[n // 2] * xs.reshape(-1)
    assert _planes_ok(data, width, n, w, False, wx * wx)
    want = pyoracle.render(edgeref.FMT, data, n, w, ps.block_norm, ps.gain, ps.rng, edgeref.lut(256), width)
    assert len(np.unique(want["gauge_amps"])) == 256


@pytest.mark.parametrize("ch", [False, True])
def test_peak_capture_lets_the_hold_decide(ch):
    """Stride exactly M * n, M sub-frames in every column but the last, and in every column the winning sub-frame is the one that
    carries the straddling value, whichever its neighbours hold: silence, x / 2 or the double below x."""
    n, m = 64, edgeref.PEAK_M
    ps = edgeref.DEFAULT
    e = edgeref.all_index_edges(ps)
    data, width, col_x, pairs = edgeref.peak_capture(e, n, edgeref.OFFSETS5, m)
    assert width == len(e) * 5 + 1 and data.size == 16 * (n + (width - 1) * m * n)
    want = peakref.expected(edgeref.FMT, data, n, edgeref.taper(n, True), ps.block_norm, ps.gain, ps.rng, edgeref.lut(ps.lut_len), width, ch)
    assert want["M"] == m and want["counts"] == [m] * (width - 1) + [1]
    top = n // 2 if ch else n
    assert (want["jstar"][:-1, :top] == np.array([j for _, j in pairs])[:, None]).all()
    # every (variant, sub-frame) pair is used about equally often, and by values on both sides of edges
    count = {}
    for (v, j), x, edge in zip(pairs, col_x, np.repeat(e, 5)):
        below, above = count.setdefault((v, j), [0, 0])
        count[(v, j)] = [below + (x * x < edge), above + (x * x >= edge)]
    assert len(count) == 3 * m and all(min(c) > 200 for c in count.values()), count
    # the column's value is x*x: the reply shows the same pixels as the single-frame capture of the same values
    single = pyoracle.render(edgeref.FMT, edgeref.straddle_capture(e, n, edgeref.OFFSETS5)[0], n, edgeref.taper(n, True), ps.block_norm,
                             ps.gain, ps.rng, edgeref.lut(ps.lut_len), width - 1, ch)
    assert np.array_equal(want["rgba"].reshape(n, width, 4)[:, :-1], single["rgba"].reshape(n, width - 1, 4))


@pytest.mark.parametrize("case", edgeref.PEAK_CASES, ids=lambda c: "%s_n%d_%s" % (c[0].name, c[1], "lr" if c[2] else "iq"))
def test_peak_edge_subsets_are_straddled(case):
    ps, n, ch = case
    e = edgeref.peak_edge_subset(ps, n)
    assert len(e) >= (1255 if n <= 256 else 313)
    assert edgeref.straddles(edgeref.straddle_values(e, edgeref.OFFSETS5), e).all()
    assert len(set(edgeref.peak_capture(e[:20], n, edgeref.OFFSETS5)[3])) == 9


def test_log10_probe_values():
    x = edgeref.log10_probe_values()
    assert len(x) == 200 and len(np.unique(x)) == 200 and (x > 0).all() and np.isfinite(x).all()
    assert (x < 1).sum() > 100 and (x > 1).sum() > 30           # dBfs_min shows the ones below 1, dBfs_max the ones above
