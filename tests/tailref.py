"""Every format's capture tail - the byte counts that are whole elements but no whole sample - as captures for every kernel family, and
what makes each of them telling.  tests/test_tails_cpu.py proves the conditions on the oracle, tests/test_tails_gpu.py runs the cases.
Test infrastructure, not a test.

A (format, tail) pair is a capture of whole samples with `tail` more bytes behind them: nbytes % elem == 0, and nbytes % sample width
== tail.  The reference reads such a capture (lib/samples.js): a typed view gives NaN past its last element, the 4-bit and 12-bit
formats read a missing byte as 0, CU64 / CS64 treat the two words of a value differently.  tests/golden/decode_tails.json pins both
oracles for all 32 pairs against the real lib/samples.js.

Two regimes put frames outside the capture:
    overhang  several whole frames, and the last frame ends past the capture.  A frame starts at ToInt32(0.5 + stride * x)
              (worker.js:72), the last one at about sampleCount - n rounded to nearest: it ends past the last whole sample exactly where
              the tail is half a sample or more (OVERHANGS).  With a shorter tail, tail 0 included, the last frame ends flush with the
              last whole sample, every frame is inside the capture and the prefetching loader serves the request with the tail bytes
              directly behind its last read: those cases are `flush`, and nothing but the reply is asserted of them.
    short     fewer samples than n, 5 frames: the stride is negative, every start after the first is below 0.
The captures lie between two guards of GUARD_BYTE, n sample widths or more each: a loader that ignores a bound reads guard bytes and
gives a wrong answer, not a fault.  as_if_in_bounds() is that wrong answer's input."""
import numpy as np

import peakref
import siggen

FORMATS = peakref.FORMATS
SW = siggen.SAMPLE_WIDTH
ELEM = {"CU4": 1, "CS4": 1, "CU8": 1, "CS8": 1, "CU12": 1, "CS12": 1, "CU16": 2, "CS16": 2, "CU32": 4, "CS32": 4, "CU64": 4, "CS64": 4,
        "CF32": 4, "CF64": 8}        # (a 64-bit value is read as two 32-bit words)
TAILS = {"CU4": (0,), "CS4": (0,), "CU8": (0, 1), "CS8": (0, 1), "CU12": (0, 1, 2), "CS12": (0, 1, 2), "CU16": (0, 2), "CS16": (0, 2),
         "CU32": (0, 4), "CS32": (0, 4), "CU64": (0, 4, 8, 12), "CS64": (0, 4, 8, 12), "CF32": (0, 4), "CF64": (0, 8)}
PAIRS = [(f, t) for f in FORMATS for t in TAILS[f]]
REFUSED = (("CS16", 1), ("CF32", 3))                 # nbytes % elem != 0: the reference throws, the library answers -3
REGIMES = ("overhang", "short")
FAMILIES = ("frames", "peak", "traces", "power", "index")          # one request each; a batch holds a format's pairs as items
SCRATCH_KINDS = ("image", "peak", "traces", "power")
SCRATCH_SIZES = (32, 2048)
PACKED = ("CU4", "CS4", "CU12", "CS12")              # a missing byte reads as 0: a half-present sample is finite
GUARD_BYTE = 0x5A
TAIL_BYTES = np.array([0xC3, 0x69, 0x96, 0x3C, 0xA7, 0x1E, 0xE1, 0x78, 0x87, 0xD2, 0x2D, 0xB4], np.uint8)      # none of them the guard's
SHORT_WIDTH = 5
WINDOW = "hamming"          # its ends are 0.08: a taper that ends in 0 (hann) would hide the one sample an overhanging frame reads past the end
GEN = {"kind": "trinoise", "seed": 20262, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
NOISY = dict(GEN, amp=0.35, namp=0.3)                # 4-bit samples: enough noise that no bin of a short frame is exactly zero


def overhangs(fmt, tail):
    """The last frame of an overhang capture ends past the capture: the tail is half a sample or more."""
    return 2 * tail >= SW[fmt]


def width_of(regime, n):
    """Frames of a request: 5 in the short regime; else 37 at n <= 64 (several frames per wave) and 9 above."""
    return SHORT_WIDTH if regime == "short" else 37 if n <= 64 else 9


def starts(fmt, n, nbytes, W):
    """Every frame's first sample in the reference's arithmetic (worker.js:72)."""
    sc = nbytes / SW[fmt]
    if W < 2:
        return [0] * W
    stride = (np.float64(sc) - n) / np.float64(W - 1)
    return [peakref.to_int32(0.5 + stride * x) for x in range(W)]


def leaving(fmt, n, nbytes, W):
    """The frames that read outside the capture."""
    return [x for x, p in enumerate(starts(fmt, n, nbytes, W)) if p < 0 or (p + n) * SW[fmt] > nbytes]


def inside(fmt, n, nbytes, W):
    return [x for x in range(W) if x not in leaving(fmt, n, nbytes, W)]


def _signal(fmt, samples, seed):
    gen = NOISY if fmt in ("CU4", "CS4") else GEN
    return siggen.generate(fmt, dict(gen, seed=gen["seed"] + seed), samples)


def capture(fmt, tail, regime, n, sparse=False, seed=0):
    """The capture of a case, u8: whole samples of trinoise and `tail` bytes of TAIL_BYTES.  sparse: 2 n samples or more per column (the
    peak detector's M = 2).  overhang: the first length at which the last frame's start rounds up where the tail allows it."""
    sw, W = SW[fmt], width_of(regime, n)
    if regime == "short":
        return np.concatenate([_signal(fmt, n // 2 + 7, seed), TAIL_BYTES[:tail]])
    samples = n + (W - 1) * 2 * n + (W - 1) // 2 + 1 if sparse else n + (W - 1) * (n // 2 + 3) + 1
    for more in range(16):
        data = np.concatenate([_signal(fmt, samples + more, seed), TAIL_BYTES[:tail]])
        if not overhangs(fmt, tail) or leaving(fmt, n, data.size, W):
            return data
    raise AssertionError("no capture of %s +%d n=%d W=%d ends inside its last frame" % (fmt, tail, n, W))


def guard_bytes(fmt, n):
    """n sample widths, rounded up to a multiple of 16 (the capture keeps the buffer's alignment), and 64 more."""
    return (n * SW[fmt] + 15) // 16 * 16 + 64


def guarded(fmt, n, data):
    """(the capture between its guards, the capture's offset in it)"""
    g = guard_bytes(fmt, n)
    return np.concatenate([np.full(g, GUARD_BYTE, np.uint8), data, np.full(g + 16, GUARD_BYTE, np.uint8)]), g


def as_if_in_bounds(fmt, n, data, start):
    """The n samples a loader that ignores the capture's bounds reads for a frame that starts at `start`: guard bytes where the frame
    leaves the capture."""
    G, g = guarded(fmt, n, data)
    sw = SW[fmt]
    assert g + start * sw >= 0 and g + (start + n) * sw <= G.size
    return G[g + start * sw:g + (start + n) * sw].copy()


# ------------------------------------------------------------------------------------------------------------------- the cases
def index_built(n, ch):
    """k_frames_index has no L/R variant of the generic loaders at n <= 256."""
    return not (ch and n <= 256)


def lattice():
    """Every (format, tail, regime) through every single-request family: 32 x 2 x 5 cases.  n alternates between 64 and 1024 over the
    families and regimes of a pair; host-fed or device-resident, the L/R split and the layout rotate over the pairs at other periods."""
    cases = []
    for pi, (fmt, tail) in enumerate(PAIRS):
        for ri, regime in enumerate(REGIMES):
            for fi, family in enumerate(FAMILIES):
                s = 10 * pi + 5 * ri + fi
                n = (64, 1024)[s % 2]
                ch = (s // 3) % 2 == 1
                if family == "index" and not index_built(n, ch):
                    ch = False
                cases.append(dict(family=family, fmt=fmt, tail=tail, regime=regime, n=n, ch=ch, wf=family in ("frames", "peak", "index") and (s // 7) % 2 == 1,
                                  host=(s // 2) % 2 == 1, sparse=family == "peak" and regime == "overhang"))
    return cases


def scratch_lattice():
    """Every (format, tail, regime) once per scratch kernel kind at n = 32 and n = 2048 (forced), device-resident."""
    cases = []
    for pi, (fmt, tail) in enumerate(PAIRS):
        for ri, regime in enumerate(REGIMES):
            for ni, n in enumerate(SCRATCH_SIZES):
                for ki, kind in enumerate(SCRATCH_KINDS):
                    s = 16 * pi + 8 * ri + 4 * ni + ki
                    cases.append(dict(family="scratch_" + kind, kind=kind, fmt=fmt, tail=tail, regime=regime, n=n, ch=(s // 3) % 2 == 1,
                                      wf=kind in ("image", "peak") and (s // 5) % 2 == 1, host=False, sparse=kind == "peak" and regime == "overhang"))
    return cases


def batches():
    """One batch per format: every tail in both regimes as an item, and one item of whole samples whose frames overlap."""
    out = []
    for k, fmt in enumerate(FORMATS):
        n = (64, 512)[k % 2]
        items = [dict(fmt=fmt, tail=t, regime=r, n=n, sparse=False) for t in TAILS[fmt] for r in REGIMES]
        out.append(dict(family="batch", fmt=fmt, n=n, ch=(k // 2) % 2 == 1, wf=(k // 3) % 2 == 1, host=(k // 4) % 2 == 1, items=items))
    return out


def case_id(c):
    if c["family"] == "batch":
        return "batch_%s_n%d%s%s_%s" % (c["fmt"], c["n"], "_lr" if c["ch"] else "", "_wf" if c["wf"] else "", "host" if c["host"] else "resident")
    return "%s_%s+%d_%s_n%d%s%s_%s" % (c["family"], c["fmt"], c["tail"], c["regime"], c["n"], "_lr" if c["ch"] else "", "_wf" if c["wf"] else "",
                                       "host" if c["host"] else "resident")


def request(c, seed=0):
    """(W, capture) of a case or of a batch's item."""
    return width_of(c["regime"], c["n"]), capture(c["fmt"], c["tail"], c["regime"], c["n"], c["sparse"], seed)


def whole_item(fmt, n):
    """The in-bounds item of a batch: (W, capture), 9 overlapping frames of whole samples."""
    W = 9
    return W, _signal(fmt, n + (W - 1) * (n // 4 + 1), 99)
