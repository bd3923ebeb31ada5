"""The burst measurements without a device: the ABI, the planted series of tests/pulseref.py (that the expected arrays show every plant
at every shape the GPU tests use), and the one decision of csrc/sp_pulse_core.h against pulseref - math.fsum and a plain loop - through
the library's host side (sp_debug_pulses) and through a stand-alone program built with the address and undefined-behaviour sanitizers
(tests/cpp/pulse_core_check.cpp), which also measures as the kernels do: 64-frame words, segments of 64, 128 and
SP_BURST_SEGMENT_FRAMES frames in a shuffled order, partial cells added in that order, one writer per stored slot."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pulseref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_plan_execute_pulses", "sp_power_pulses", "sp_series_pulses", "sp_render_pulses", "sp_plan_pulses_kernel_name_for",
                "sp_debug_pulses")
TAIL = "double *%senergy, double *%speak, int32_t *%speak_at);"


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def _segment():
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    return int(re.search(r"^#define SP_BURST_SEGMENT_FRAMES (\d+)$", hdr, re.M).group(1))


def gpu_widths(S):
    return (1, 2, 63, 64, 65, 257, S - 1, S, S + 1, 2 * S + 3, 64 * S + 5)


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    flat = " ".join(hdr.split())
    d = ("d_",) * 3
    for decl in ("int sp_plan_execute_pulses(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, "
                 "int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, " + TAIL % d,
                 "int sp_power_pulses(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, "
                 "const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, " + TAIL % d,
                 "int sp_series_pulses(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, "
                 "const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, " + TAIL % d,
                 "int sp_render_pulses(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, "
                 "const int32_t *bands, int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *counts, "
                 "int32_t *edges, " + TAIL % ("", "", ""),
                 "const char *sp_plan_pulses_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);",
                 "int sp_debug_pulses(const double *values, int32_t width, double hi, double lo, int32_t max_bursts, uint32_t *count_out, "
                 "int32_t *edges_out, double *energy_out, double *peak_out, int32_t *peak_at_out);"):
        assert decl in flat, decl
    assert hdr.index("Burst lists:") < hdr.index("Burst measurements:") < hdr.index("Indexed image replies:")
    text = hdr[hdr.index("Burst measurements:"):hdr.index("int sp_plan_execute_pulses")]
    for word in ("SP_ERR_UNSUPPORTED", "SP_ERR_INVALID_ARG", "SP_ERR_NOMEM", "math.fsum", "rounded ONCE", "0x7ff8000000000000", "EARLIEST",
                 "0xFF BYTES", "8-byte aligned", "4-byte aligned", "sp_pulse_core.h", "SP_BURST_SEGMENT_FRAMES", "8 * 68 * count * max_bursts",
                 "8 * count * max_bursts", "No workgroup waits", "UNSIGNED", "Out of scope", "rows[b][peak_at]", "not measured"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_pulses", "pulses_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_pulses", "power_pulses", "series_pulses"):
        assert hasattr(pkg.Context, name), name
    assert callable(pkg.pulse_scan) and "pulse_scan" in pkg.__all__
    b = pkg.binding
    # no existing structure changed
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.SP_MAX_BANDS == 64 and b.SP_BURST_SEGMENT_FRAMES == _segment()


def test_refusals_without_a_device(pkg):
    """Every refusal that can be reached without a context: null handles, and through sp_debug_pulses - which checks its thresholds and
    outputs with the functions every entry point checks them with - the burst lists' refusals in their order, every output absent,
    per-burst outputs with max_bursts == 0, and misaligned outputs.  A refusal writes nothing."""
    L = pkg.Library.get().L
    one = (C.c_double * 1)(1.0)
    band = (C.c_int32 * 2)(0, 1)
    cnt = (C.c_uint32 * 4)()
    pc = C.cast(cnt, C.c_void_p)
    assert L.sp_plan_execute_pulses(None, None, 0, 0, band, 1, one, one, 1, pc, None, None, None, None) == -1
    assert L.sp_power_pulses(None, None, 4, 0, band, 1, one, one, 1, pc, None, None, None, None) == -1
    assert L.sp_series_pulses(None, None, 1, 0, one, one, 1, pc, None, None, None, None) == -1
    assert L.sp_render_pulses(None, None, None, 0, 0, band, 1, one, one, 1, pc, None, None, None, None) == -1
    assert L.sp_plan_pulses_kernel_name_for(None, 0, 0) == b""
    v = np.array([0.0, 9.0, 9.5, 0.0])
    pv = v.ctypes.data_as(C.c_void_p)
    total = C.c_uint32(77)
    edges = np.full(5, 0x55555555, np.int32)
    energy, peak = np.full(3, 1234.5), np.full(3, 1234.5)
    at = np.full(3, 0x55555555, np.int32)
    pe, pn, pp, pa = (C.c_void_p(a.ctypes.data) for a in (edges, energy, peak, at))
    dbg = L.sp_debug_pulses
    for hi, lo in ((math.nan, 1.0), (2.0, math.nan), (1.0, 2.0), (0.0, 5e-324), (-3.0, 1.0)):   # NaN; lo > hi by key
        assert dbg(pv, 4, hi, lo, 2, C.byref(total), pe, pn, pp, pa) == -1, (hi, lo)
    assert dbg(pv, 4, 2.0, 1.0, 2, None, None, None, None, None) == -1                 # every output absent
    assert dbg(pv, 4, 2.0, 1.0, 0, None, pe, pn, pp, pa) == -1                         # per-burst outputs with max_bursts == 0 are absent
    assert dbg(pv, 4, 2.0, 1.0, -1, C.byref(total), pe, pn, pp, pa) == -1              # max_bursts < 0
    off = lambda a, k: C.c_void_p(a.ctypes.data + k)  # noqa: E731
    assert dbg(pv, 4, 2.0, 1.0, 2, C.byref(total), off(edges, 2), pn, pp, pa) == -1    # misaligned edges
    assert dbg(pv, 4, 2.0, 1.0, 2, C.byref(total), pe, off(energy, 4), pp, pa) == -1   # energy is 8-byte aligned
    assert dbg(pv, 4, 2.0, 1.0, 2, C.byref(total), pe, pn, off(peak, 4), pa) == -1     # ... and peak
    assert dbg(pv, 4, 2.0, 1.0, 2, C.byref(total), pe, pn, pp, off(at, 2)) == -1       # peak_at is 4-byte aligned
    assert dbg(pv, 4, 2.0, 1.0, 2, C.cast(C.c_void_p(C.addressof(cnt) + 1), C.POINTER(C.c_uint32)), pe, pn, pp, pa) == -1
    assert dbg(None, 4, 2.0, 1.0, 2, C.byref(total), pe, pn, pp, pa) == -1
    assert dbg(pv, -1, 2.0, 1.0, 2, C.byref(total), pe, pn, pp, pa) == -1
    assert total.value == 77 and (edges == 0x55555555).all() and (energy == 1234.5).all() and (peak == 1234.5).all() and (at == 0x55555555).all()
    # what is no refusal: each output alone, and counts alone with max_bursts == 0
    assert dbg(pv, 4, 2.0, 2.0, 2, None, None, pn, None, None) == 0
    assert energy[0] == 18.5 and energy[:2].view(np.uint64)[1] == pulseref.FILL_BITS and energy[2] == 1234.5
    assert dbg(pv, 4, 2.0, 2.0, 2, None, None, None, pp, None) == 0 and peak[0] == 9.5 and peak[2] == 1234.5
    assert dbg(pv, 4, 2.0, 2.0, 2, None, None, None, None, pa) == 0 and at.tolist() == [2, -1, 0x55555555]
    assert dbg(pv, 4, 2.0, 2.0, 0, C.byref(total), pe, pn, pp, pa) == 0 and total.value == 1
    assert dbg(None, 0, 2.0, 1.0, 2, C.byref(total), pe, pn, pp, pa) == 0 and total.value == 0 and at.tolist() == [-1, -1, 0x55555555]
    with pytest.raises(pkg.SpectroplotError) as e:
        pkg.pulse_scan(v, 1.0, 2.0, 2)
    assert e.value.status == -1


def test_reference_on_hand_checked_series():
    nan, inf = math.nan, math.inf
    for row, hi, lo, want in (
            ([], 8, 2, []), ([9], 8, 2, [(0, 1, 9.0, 9.0, 0)]), ([nan], 8, 2, []),
            ([0, 8, 5, 2, nan, 1.9, 8], 8, 2, [(1, 5, nan, 8.0, 1), (6, 7, 8.0, 8.0, 6)]),
            ([9, 9, 0, 0, inf, 5], 8, 2, [(0, 2, 18.0, 9.0, 0), (4, 6, inf, inf, 4)]),
            ([9, 10, 10, 0], 8, 2, [(0, 3, 29.0, 10.0, 1)]),
            ([1e308, 1e308, 0], 8, 2, [(0, 2, inf, 1e308, 0)]),
            ([2.0 ** 53, 1.0, 1.0], 8, -1, [(0, 3, 2.0 ** 53 + 2, 2.0 ** 53, 0)]),
            ([-9.0, 3, -10.0], 8, 2, [(0, 3, 22.0, 10.0, 2)])):      # read by key: the sign bit is not looked at
        got = pulseref.measure(np.array(row, np.float64), hi, lo)
        assert len(got) == len(want), row
        for g, w in zip(got, want):
            assert g[:2] == w[:2] and g[4] == w[4] and g[3] == w[3] and (g[2] == w[2] or (g[2] != g[2] and w[2] != w[2])), (row, g, w)
    reply = pulseref.expected(np.array([[1, 9, 1, 9, 1, 9.0], [0, 0, 0, 0, 0, 0]]), [8, 8], [2, 2], 2)
    counts, edges, energy, peak, peak_at = reply
    assert counts.tolist() == [3, 0] and edges.tolist() == [[[1, 2], [3, 4]], [[-1, -1], [-1, -1]]]
    assert energy.dtype == peak.dtype == np.uint64 and peak_at.dtype == np.int32
    assert energy[0].view(np.float64).tolist() == [9.0, 9.0] and (energy[1] == pulseref.FILL_BITS).all() and peak_at.tolist() == [[1, 3], [-1, -1]]
    small = pulseref.cut(reply, 1)
    assert small[0].tolist() == [3, 0] and small[2].shape == (2, 1) and small[4].tolist() == [[1], [-1]]


def test_planted_series_tell_at_every_shape_the_tests_use():
    """Asserted on the reference's output, not the library's: the expected arrays show every plant the shape has room for - at the GPU
    tests' shapes and at the segment sizes of the stand-alone program - and a left-to-right float sum gets a planted burst wrong."""
    S = _segment()
    everything = set()
    for seg in (64, 128, S):
        for seed in (0, 1):
            for count in (1, 6):
                for width in gpu_widths(S)[:-1] + ((gpu_widths(S)[-1],) if (seg, seed, count) == (S, 0, 6) else ()):
                    got, need = pulseref.telling(seed, count, width, seg), pulseref.must_tell(seed, count, width, seg)
                    assert need <= got, (seg, seed, count, width, sorted(need - got))
                    everything |= got
    all_plants = set(pulseref._plants(S)) | {"nan_inside_a_burst", "inf_frame", "open_at_width", "alternating", "never_bursts",
                                             "across_three_segments"}
    assert everything == all_plants and len(all_plants) == 16, sorted(all_plants ^ everything)
    assert pulseref.must_tell(0, 6, 64 * S + 5, S) == all_plants          # the widest shape holds every one of them
    assert "naive_fails" in pulseref.must_tell(0, 6, 63, S)
    # the long burst of band 4, hundreds of addends over the whole exponent range: the float sum is off there, too
    series, hi, lo = pulseref.planted_series(0, 6, 2 * S + 3, S)
    counts, edges, energy, _, _ = pulseref.planted_expected(0, 6, 2 * S + 3, S)
    assert counts[4] == 1 and edges[4, 0].tolist() == [3, 2 * S + 3]
    assert pulseref.bits_of(pulseref.naive_sum(series[4, 3:])) != energy[4, 0]
    assert counts[1] == (2 * S + 3) // 2 and counts[2] == 0


def _cases(S):
    """(series row, hi, lo, max_bursts): every band of planted series at small widths and 200 random series over the whole range."""
    out = []
    for seed in (0, 1):
        for width in (1, 2, 63, 64, 65, 257, 2 * S + 3):
            series, hi, lo = pulseref.planted_series(seed, 6, width, 64 if width < 2 * S else S)
            for b in range(6):
                for m in ((0, 1, 7, width // 2 + 1) if seed == 0 and width <= 257 else (7,)):
                    out.append((series[b], hi[b], lo[b], m))
    rng = np.random.default_rng(2028)
    vals = np.array([0.0, 1.0, 2.0, 5.0, 8.0, 9.0, 2.0 ** 53, 2.0 ** 53 + 2, 1e300, 1.7e308, math.inf, math.nan, -9.0, 5e-324, 2.0 ** -1022])
    for i in range(200):
        width = int(rng.choice([0, 1, 5, 64, 130, 700]))
        row = rng.choice(vals, width) if i % 2 else meanref_values(rng, width)
        hi, lo = ((8.0, 2.0), (5.0, 5.0), (8.0, -1.0), (math.inf, 2.0), (2.0, 0.0), (0.0, 0.0))[i % 6]
        out.append((row, hi, lo, int(rng.choice([0, 1, 3, width // 2 + 1]))))
    return out


def meanref_values(rng, width):
    import meanref
    return meanref.random_values(rng, width, clustered=bool(rng.integers(0, 2))) if width else np.zeros(0)


def _want(row, hi, lo, m):
    counts, edges, energy, peak, peak_at = pulseref.expected(np.asarray(row, np.float64)[None, :], [hi], [lo], m)
    return int(counts[0]), edges[0], energy[0], peak[0], peak_at[0]


def test_debug_pulses_against_the_reference(pkg):
    checked = cut = none = nans = infs = 0
    for row, hi, lo, m in _cases(_segment()):
        total, edges, energy, peak, peak_at = pkg.pulse_scan(row, hi, lo, m)
        want = _want(row, hi, lo, m)
        what = (len(row), hi, lo, m)
        assert total == want[0] and np.array_equal(edges, want[1]), what
        assert energy.dtype == np.float64 and np.array_equal(energy.view(np.uint64), want[2]), what
        assert np.array_equal(peak.view(np.uint64), want[3]) and peak_at.dtype == np.int32 and np.array_equal(peak_at, want[4]), what
        total_b, edges_b = pkg.burst_scan(row, hi, lo, m)
        assert total_b == total and np.array_equal(edges_b, edges), what        # the bursts are sp_debug_bursts'
        checked += 1
        cut += total > m
        none += total == 0
        nans += bool((want[2] == pulseref.NAN_BITS).any())
        infs += bool((want[2] == pulseref.bits_of(math.inf)).any())
    assert checked > 250 and cut > 40 and none > 20 and nans > 10 and infs > 10


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/sp_pulse_core.h alone, host compiler, -fsanitize=address,undefined, the runtimes linked in: the same series through stdin,
    measured by the host loop and as the kernels measure; the answers against pulseref."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pulse_core_check")
    csrc = os.path.join(ROOT, "spectroplot-js_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # (the runtimes linked in)
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "pulse_core_check.cpp")])
    S = _segment()
    cases = _cases(S)
    series, hi, lo = pulseref.planted_series(0, 6, 5 * S + 70, S)       # the three-segment burst and its equal maxima at the real size
    cases += [(series[b], hi[b], lo[b], m) for b in range(6) for m in (7, 5 * S)]
    series, hi, lo = pulseref.planted_series(1, 6, 64 * 128 + 5, 128)
    cases += [(series[b], hi[b], lo[b], 5000) for b in range(6)]
    bits = lambda v: "%016x" % np.array([v], np.float64).view(np.uint64)[0]  # noqa: E731
    lines, want = [], []
    for row, h, l, m in cases:
        row = np.ascontiguousarray(row, np.float64)
        lines.append("%s %s %d %d %s" % (bits(h), bits(l), m, len(row), " ".join("%x" % b for b in row.view(np.uint64).tolist())))
        total, edges, energy, peak, peak_at = _want(row, h, l, m)
        want.append(" ".join([str(total)] + [str(v) for v in edges.reshape(-1).tolist()] + ["%x" % v for v in energy.tolist()]
                             + ["%x" % v for v in peak.tolist()] + [str(v) for v in peak_at.tolist()]))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(want) + 1 and got[-1] == ""
    for line, g, w in zip(lines, got, want):
        assert g == w, (line[:80], g[:200], w[:200])
