"""Capture tails without a device: the C oracle against tests/golden/decode_tails.json (vectors of the real lib/samples.js for all 32
(format, tail) pairs; oracle/js/check_golden.js checks the JS oracle against the same file), the case lists of tests/tailref.py, and
the proof that every case is telling: at every frame that leaves the capture the oracle's reply differs from what a loader that ignores
the capture's bounds - and reads the guard bytes around it - would produce."""
import functools
import json
import os

import numpy as np
import pytest

import siggen
import tailref
import variantref
from goldenlib import f64_from_hex, same_f64
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)
GAIN, RANGE = 6.0, 50.0
CASES, SCRATCH, BATCHES = tailref.lattice(), tailref.scratch_lattice(), tailref.batches()


@functools.lru_cache(maxsize=None)
def _fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "decode_tails.json")))


def test_the_fixture_holds_every_pair_and_the_two_refused_counts():
    D = _fixture()
    assert [(e["format"], e["tail"]) for e in D if "throws" not in e] == tailref.PAIRS and len(tailref.PAIRS) == 32
    assert [(e["format"], e["tail"]) for e in D if "throws" in e] == list(tailref.REFUSED)
    for e in D:
        sw, elem = siggen.SAMPLE_WIDTH[e["format"]], tailref.ELEM[e["format"]]
        assert e["bytes"] % sw == e["tail"] and 24 <= e["bytes"] <= 48
        assert (e["bytes"] % elem != 0) == ("throws" in e)
        if "throws" not in e:
            assert e["pos_lo"] == -3 and e["pos_hi"] > e["bytes"] // sw + 2 and len(e["values"]) == 2 * (e["pos_hi"] - e["pos_lo"])
    # valid tails by the rule: whole elements, no whole sample
    for fmt in tailref.FORMATS:
        sw, elem = siggen.SAMPLE_WIDTH[fmt], tailref.ELEM[fmt]
        assert tailref.TAILS[fmt] == tuple(t for t in range(sw) if t % elem == 0), fmt


@pytest.mark.parametrize("k", range(34), ids=lambda k: _fixture()[k]["name"])
def test_c_oracle_decodes_the_tail_as_the_reference_does(k):
    e = _fixture()[k]
    sw = siggen.SAMPLE_WIDTH[e["gen_format"]]
    data = siggen.generate(e["gen_format"], {"kind": "bytes", "seed": e["seed"]}, -(-e["bytes"] // sw))[:e["bytes"]]
    if "throws" in e:
        with pytest.raises(pyoracle.OracleError):
            pyoracle.decode(e["format"], data, 0, 1)
        return
    vals, count, width = pyoracle.decode(e["format"], data, e["pos_lo"], e["pos_hi"] - e["pos_lo"])
    assert width == e["sampleWidth"] == sw and same_f64(count, e["sampleCount"])
    flat = vals.reshape(-1)
    assert len(flat) == len(e["values"])
    for j, (v, h) in enumerate(zip(flat, e["values"])):
        assert same_f64(float(v), h), (e["name"], e["pos_lo"] + j // 2, "IQ"[j % 2], v, f64_from_hex(h))


def test_the_tail_rules_are_in_the_vectors():
    """What the issue names: a typed view gives NaN past its last element - also for the half sample whose I is present -, the packed
    formats read missing bytes as 0 so that their half-present sample is finite, CS64's missing high word reads 0.0 next to a NaN low."""
    D = {e["name"]: e for e in _fixture()}

    def iq(name, pos):
        e = D[name]
        j = 2 * (pos - e["pos_lo"])
        return f64_from_hex(e["values"][j]), f64_from_hex(e["values"][j + 1])

    for fmt, tail in tailref.PAIRS:
        e = D["tail_%s_%d" % (fmt, tail)]
        whole = e["bytes"] // siggen.SAMPLE_WIDTH[fmt]
        i, q = iq(e["name"], whole)                 # the half-present sample (tail 0: the first sample past the end)
        i2, q2 = iq(e["name"], whole + 2)
        ib, qb = iq(e["name"], -2)
        if fmt in tailref.PACKED:
            assert all(np.isfinite(v) for v in (i, q, i2, q2, ib, qb)), e["name"]
        elif fmt in ("CU64", "CS64"):
            # a value is (low word, high word): a missing low word is NaN, a missing high word NaN for CU64 and 0.0 for CS64 - so CS64's
            # value is finite exactly where its low word alone is present (+4: I, +12: Q)
            assert all(np.isnan(v) for v in (i2, q2, ib, qb)), e["name"]
            assert np.isfinite(i) == (tail >= 8 or (tail == 4 and fmt == "CS64")), e["name"]
            assert np.isfinite(q) == (tail == 12 and fmt == "CS64"), e["name"]
        else:
            assert np.isnan(q) and np.isnan(i2) and np.isnan(q2) and np.isnan(ib) and np.isnan(qb), e["name"]
            assert np.isnan(i) == (tail == 0), e["name"]          # I of the half sample is there
        if fmt not in tailref.PACKED and tail and 2 * tail >= siggen.SAMPLE_WIDTH[fmt] and fmt not in ("CU64", "CS64"):
            assert np.isfinite(i) or fmt in ("CF32", "CF64")      # (random bytes can spell a NaN float)


def test_what_the_lattices_cover():
    assert len(CASES) == 32 * 2 * 5 and len(SCRATCH) == 32 * 2 * 2 * 4 and len(BATCHES) == 14
    ids = [tailref.case_id(c) for c in CASES + SCRATCH + BATCHES]
    assert len(set(ids)) == len(ids)
    assert sum(len(b["items"]) for b in BATCHES) == 32 * 2
    for fmt in tailref.FORMATS:
        mine = [c for c in CASES if c["fmt"] == fmt]
        assert {c["host"] for c in mine} == {False, True} and {c["n"] for c in mine} == {64, 1024} and {c["ch"] for c in mine} == {False, True}, fmt
        for tail in tailref.TAILS[fmt]:
            for regime in tailref.REGIMES:
                cell = [c for c in mine if c["tail"] == tail and c["regime"] == regime]
                assert [c["family"] for c in cell] == list(tailref.FAMILIES)
                assert {c["host"] for c in cell} == {False, True} and {c["n"] for c in cell} == {64, 1024}
    for family in tailref.FAMILIES:
        mine = [c for c in CASES if c["family"] == family]
        assert {(c["n"], c["host"]) for c in mine} == {(64, False), (64, True), (1024, False), (1024, True)}, family
        assert {c["regime"] for c in mine} == set(tailref.REGIMES)
        if family in ("frames", "peak", "index"):
            assert {c["wf"] for c in mine} == {False, True}
    assert {b["n"] for b in BATCHES} == {64, 512} and {b["host"] for b in BATCHES} == {False, True}
    # the pairs that can overhang: a tail of half a sample or more - 14 of the 32; the other 18 end flush
    assert sum(tailref.overhangs(f, t) for f, t in tailref.PAIRS) == 14


CAPTURES = sorted({(c["fmt"], c["tail"], c["regime"], c["n"], c["sparse"]) for c in CASES + SCRATCH}
                  | {(i["fmt"], i["tail"], i["regime"], i["n"], False) for b in BATCHES for i in b["items"]})


def _planes(fmt, data, n, W):
    win, weight = pyoracle.window(tailref.WINDOW, n)
    assert win[0] != 0.0 and win[-1] != 0.0
    return pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, LUT, W, False, False, planes=True)["abs2"]


def _differ(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na != nb).any() or (a[~na] != b[~nb]).any())


@pytest.mark.parametrize("key", CAPTURES, ids=["%s+%d_%s_n%d%s" % (k[0], k[1], k[2], k[3], "_sparse" if k[4] else "") for k in CAPTURES])
def test_every_capture_is_telling(key):
    """At every frame that leaves the capture the oracle's frame differs from the frame read through the guards as if in bounds; the packed
    formats' leaving frames are finite and no all-zero frame; an overhang capture keeps 3 frames or more wholly inside; a capture that
    cannot overhang is flush: every frame inside, the prefetching loader's."""
    fmt, tail, regime, n, sparse = key
    sw = siggen.SAMPLE_WIDTH[fmt]
    W = tailref.width_of(regime, n)
    data = tailref.capture(fmt, tail, regime, n, sparse)
    assert data.size % sw == tail and data.size % tailref.ELEM[fmt] == 0
    assert tailref.guard_bytes(fmt, n) >= n * sw and not (tailref.TAIL_BYTES == tailref.GUARD_BYTE).any()
    out = tailref.leaving(fmt, n, data.size, W)
    p = tailref.starts(fmt, n, data.size, W)
    if regime == "short":
        assert data.size // sw < n and W == 5 and out == list(range(W)) and all(s < 0 for s in p[1:]) and p[0] == 0
        assert variantref.prefetch_width(fmt, n, data.size, W) == 0
    elif tailref.overhangs(fmt, tail):
        assert out == [W - 1] and len(tailref.inside(fmt, n, data.size, W)) >= 3 and p[-1] + n == data.size // sw + 1
        assert variantref.prefetch_width(fmt, n, data.size, W) == 0
    else:
        assert out == [] and p[-1] + n == data.size // sw
        assert variantref.prefetch_width(fmt, n, data.size, W) == (sw if sw <= 8 else 0)
    if sparse:
        assert (data.size / sw - n) / (W - 1) >= 2 * n
    true = _planes(fmt, data, n, W)
    zero = _planes(fmt, np.zeros(n * sw, np.uint8), n, 1)[0]
    for x in out:
        as_if = _planes(fmt, tailref.as_if_in_bounds(fmt, n, data, p[x]), n, 1)[0]
        assert _differ(true[x], as_if), (key, x)
        if fmt in tailref.PACKED:
            assert np.isfinite(true[x]).all() and true[x].any() and _differ(true[x], zero), (key, x)
    for x in tailref.inside(fmt, n, data.size, W):              # (and the as-if reading is the oracle's own where the frame is inside)
        if x in (0, W - 2):
            assert not _differ(true[x], _planes(fmt, tailref.as_if_in_bounds(fmt, n, data, p[x]), n, 1)[0]), (key, x)
