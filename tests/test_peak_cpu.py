"""The peak detector without a device: the sub-frame rule of sp_peak_subframes against a Python restatement, the expected-value
construction the GPU tests use (tests/peakref.py) against the oracle where the two must agree, the ABI, and the compiled k_frames_peak
variants with their register / spill table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import isa
import peakref
import siggen
from __graft_entry__ import ROOT, build, load_package
from oracle import pyoracle


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def test_subframe_rule_matches_the_python_restatement_on_random_shapes(pkg):
    rng = np.random.default_rng(2027)
    held = 0
    for case in range(4000):
        fmt = peakref.FORMATS[int(rng.integers(0, 14))]
        sw = peakref.SW[fmt]
        n = 1 << int(rng.integers(1, 12))
        width = int(rng.choice([0, 1, 2, 3, int(rng.integers(2, 300))]))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            samples = int(rng.integers(0, n))                                            # shorter than a frame
        elif kind == 1:
            samples = n + max(width - 1, 0) * n * int(rng.integers(2, 9))                # integer stride, a multiple of n
        elif kind == 2:
            samples = n + max(width - 1, 0) * 2 * n + int(rng.integers(-3, 4))           # around stride = 2n: M flips 1 -> 2
        elif kind == 3:
            samples = int(rng.integers(n, n + max(width, 1) * n * 9))                    # fractional strides
        else:
            samples = int(rng.integers(n, 4 * n + width * n // 2 + 1))                   # dense / overlapping
        nbytes = max(samples, 0) * sw
        if sw == 3 and rng.integers(0, 2):
            nbytes += int(rng.integers(1, 3))                                            # a fractional sampleCount
        M, counts = peakref.subframe_rule(fmt, n, nbytes, width)
        m, last = pkg.binding.peak_subframes(fmt, n, nbytes, width)
        assert m == M, (case, fmt, n, nbytes, width, m, M)
        assert last == (counts[-1] if counts else 0), (case, fmt, n, nbytes, width, last, counts[-3:])
        if M >= 2:
            held += 1
            assert all(c == M for c in counts[:-1]), (case, fmt, n, nbytes, width)       # columns 0 .. width-2 are complete
            sample_count = nbytes / sw
            stride = (sample_count - n) / (width - 1)
            for x in (0, (width - 2) // 2, width - 2):                                        # ... and every sub-frame lies inside the capture
                assert 0 <= int(0.5 + stride * x) and int(0.5 + stride * x) + M * n <= sample_count
        else:
            assert all(c == 1 for c in counts)
    assert held > 800


def test_subframe_rule_rejects_bad_arguments(pkg):
    L = pkg.Library.get().L
    m, last = C.c_int32(), C.c_int32()
    assert L.sp_peak_subframes(99, 64, 1000, 4, C.byref(m), C.byref(last)) == -1
    assert L.sp_peak_subframes(2, 64, 1000, -1, C.byref(m), C.byref(last)) == -1
    assert L.sp_peak_subframes(2, 64, 1000, 0, C.byref(m), C.byref(last)) == 0 and (m.value, last.value) == (1, 0)
    assert L.sp_peak_subframes(2, 64, 1000, 4, None, None) == 0


def _lut(L=256):
    lut = np.stack([np.arange(L) & 255, (np.arange(L)[::-1]) & 255, (np.arange(L) * 3) & 255], axis=1).astype(np.uint8)
    lut[0] = 0
    lut[-1] = 255
    return lut


@pytest.mark.parametrize("fmt,n,width,samples,ch,wf", [
    ("CU8", 64, 37, 64 + 36 * 100, False, False),        # stride 100 < 2n: M = 1
    ("CF32", 128, 21, 128 + 20 * 255, True, True),       # just below 2n
    ("CS16", 32, 1, 500, False, False),                  # one column
    ("CS12", 64, 9, 300, False, True),                   # overlapping frames
])
def test_expected_value_construction_is_the_oracle_for_one_subframe(fmt, n, width, samples, ch, wf):
    gen = {"kind": "trinoise", "seed": 77, "step": 911, "gshift": 9, "amp": 0.4, "namp": 0.05}
    data = siggen.generate(fmt, gen, samples)
    win, weight = pyoracle.window("hann", n)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, 3.0, 40.0, _lut(), width, ch, wf)
    got = peakref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 40.0, _lut(), width, ch, wf)
    assert got["M"] == 1
    peakref.assert_same(got, want, "M = 1")


def test_expected_value_construction_holds_the_larger_subframe():
    """Two sub-frames per column, the second one louder: every pixel comes from plane 1 except in the last column, which has one."""
    n, width = 64, 5
    samples = n + (width - 1) * 2 * n
    data = np.full(2 * samples, 128, np.uint8)
    t = np.arange(samples)
    loud = ((t // n) % 2) == 1
    data[0::2] = np.where(loud, 128 + 100 * np.cos(2 * np.pi * 5 * t / n), 128 + 3 * np.cos(2 * np.pi * 5 * t / n)).astype(np.uint8)
    win, weight = pyoracle.window("hann", n)
    got = peakref.expected("CU8", data, n, win, 1.0 / weight, 0.0, 60.0, _lut(), width)
    assert got["M"] == 2 and got["counts"] == [2, 2, 2, 2, 1]
    assert (got["jstar"][:-1, 5] == 1).all() and (got["jstar"][-1] == 0).all()
    lone = pyoracle.render("CU8", data, n, win, 1.0 / weight, 0.0, 60.0, _lut(), width)
    assert got["dBfs_max"] > lone["dBfs_max"] + 10      # (the tone is 30 dB louder; the lone frames are dominated by their DC offset)


def test_request_abi_and_binding_checks(pkg):
    b = pkg.binding
    assert b._Request.detector.offset == 20 and b._Request.detector.size == 4 and b._Request.block_norm.offset == 24
    assert b.DETECTORS == {"sample": 0, "peak": 1}
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    assert re.search(r"enum sp_detector \{ SP_DETECTOR_SAMPLE = 0, SP_DETECTOR_PEAK = 1 \}", hdr)
    assert "int32_t detector;" in hdr and "int32_t reserved;\n    double block_norm" not in hdr
    L = C.CDLL(pkg.lib_path())
    for name in ("sp_peak_subframes", "sp_render_named_ex", "sp_plan_kernel_name_for"):
        assert hasattr(L, name), name
    with pytest.raises(pkg.SpectroplotError) as e:
        b._make_request(2, 64, np.ones(64), 1.0, 0.0, 30.0, _lut(), False, False, "rms")
    assert e.value.status == -1


# VGPRs and spilled VGPRs of every k_frames_peak<LOG2N, CH, PFB>: loaders 1, 2, 3, 4, 8 bytes, then the generic one
PEAK_SPILLS = {
    (6, False): [(235, 0), (235, 0), (237, 0), (235, 0), (227, 0), (256, 57)], (6, True): [(249, 0), (249, 0), (251, 0), (249, 0), (249, 0), (256, 52)],
    (7, False): [(247, 0), (247, 0), (249, 0), (247, 0), (239, 0), (256, 59)], (7, True): [(256, 0), (256, 0), (256, 0), (256, 0), (255, 0), (256, 55)],
    (8, False): [(251, 0), (251, 0), (253, 0), (251, 0), (243, 0), (256, 60)], (8, True): [(256, 3), (256, 3), (256, 3), (256, 3), (256, 3), (256, 63)],
    (9, False): [(223, 0), (223, 0), (225, 0), (223, 0), (239, 0), (256, 67)], (9, True): [(256, 17), (256, 15), (256, 15), (256, 15), (256, 19), (256, 83)],
    (10, False): [(245, 0), (245, 0), (245, 0), (245, 0), (245, 0), (256, 68)], (10, True): [(256, 22), (256, 22), (256, 22), (256, 22), (256, 23), (256, 86)],
}


def test_k_frames_peak_variants_exist_with_the_documented_spill_table():
    objs = isa.peak_objs()
    seen = {}
    for o in objs:
        for blk in isa.notes(o).split(".name:")[1:]:
            m = re.match(r"\s*_ZN4spk213k_frames_peakILi(\d+)ELb([01])ELi(\d+)E", blk)
            if not m:
                continue
            key = (int(m.group(1)), m.group(2) == "1", int(m.group(3)))
            priv = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
            spill = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1))
            vgpr = int(re.search(r"\.vgpr_count:\s*(\d+)", blk).group(1))
            seen[key] = (vgpr, spill, priv)
    assert sorted(seen) == sorted((lg, ch, p) for lg in range(6, 11) for ch in (False, True) for p in (0, 1, 2, 3, 4, 8))
    for (lg, ch, p), (vgpr, spill, priv) in seen.items():
        want = PEAK_SPILLS[(lg, ch)][(1, 2, 3, 4, 8, 0).index(p)]
        assert (vgpr, spill) == want, ((lg, ch, p), (vgpr, spill), want)
        if not ch and p:          # the variants the measured shapes run: no scratch memory at all inside the sub-frame loop
            assert priv == 0 and spill == 0, ((lg, ch, p), priv, spill)
    # no object of the sample detector's kernels holds a peak kernel, and the other way round
    for o in isa.frame_objs():
        assert "k_frames_peak" not in isa.notes(o)
    for o in objs:
        assert "_ZN4spk28k_framesI" not in isa.notes(o)
