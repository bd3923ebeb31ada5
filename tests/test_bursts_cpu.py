"""The burst lists without a device: the ABI, the planted series of tests/burstref.py (that its expected bursts show every planted
condition at every shape the GPU tests use), and the one decision of csrc/sp_burst_core.h against burstref - a plain loop of
floating-point compares - through the library's host side (sp_debug_bursts) and through a stand-alone program built with the address
and undefined-behaviour sanitizers (tests/cpp/burst_core_check.cpp), which also scans as the kernels do: 64-frame words, a summary
per segment of 64, 128 and SP_BURST_SEGMENT_FRAMES frames, the exclusive combine scan, the emit with popcounts."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import burstref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_plan_execute_bursts", "sp_power_bursts", "sp_series_bursts", "sp_render_bursts", "sp_plan_bursts_kernel_name_for",
                "sp_debug_bursts")


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
    for decl in ("int sp_plan_execute_bursts(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, "
                 "int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges);",
                 "int sp_power_bursts(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, "
                 "const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges);",
                 "int sp_series_bursts(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, "
                 "const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges);",
                 "int sp_render_bursts(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, "
                 "const int32_t *bands, int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *counts, "
                 "int32_t *edges);",
                 "const char *sp_plan_bursts_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);",
                 "int sp_debug_bursts(const double *values, int32_t width, double hi, double lo, int32_t max_bursts, uint32_t *count_out, "
                 "int32_t *edges_out);"):
        assert decl in flat, decl
    text = hdr[hdr.index("Burst lists:"):hdr.index("#define SP_BURST_SEGMENT_FRAMES")]
    for word in ("SP_ERR_UNSUPPORTED", "SP_ERR_INVALID_ARG", "SP_ERR_NOMEM", "HOST arrays", "SET", "RESET", "HOLD", "EVERY NaN", "STARTS OFF",
                 "end = width", "EVERY SLOT BEHIND THAT IS -1", "NOR ON THE CU COUNT", "sp_burst_core.h", "lo_key > hi_key", "31 bits",
                 "4-byte", "SP_MAX_BANDS", "Out of scope", "SP_BURST_SEGMENT_FRAMES", "8 * count * width", "No workgroup waits"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_bursts", "bursts_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_bursts", "power_bursts", "series_bursts"):
        assert hasattr(pkg.Context, name), name
    assert callable(pkg.burst_scan) and callable(pkg.burst_pulses)
    b = pkg.binding
    S = _segment()
    assert b.SP_BURST_SEGMENT_FRAMES == S and S % 512 == 0
    # no existing structure changed
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.DETECTORS == {"sample": 0, "peak": 1} and b.SP_MAX_BANDS == 64


def test_refusals_without_a_device(pkg):
    """Every refusal that can be reached without a context: null handles, and through sp_debug_bursts - which checks its thresholds
    and outputs with the functions every entry point checks them with - a NaN threshold, lo > hi, both outputs absent, a negative
    max_bursts and misaligned outputs.  (A context needs a device: what the entry points refuse of bands, thresholds and outputs
    with one is tests/test_bursts_gpu.py's.)"""
    L = pkg.Library.get().L
    one = (C.c_double * 1)(1.0)
    band = (C.c_int32 * 2)(0, 1)
    cnt = (C.c_uint32 * 4)()
    pc = C.cast(cnt, C.c_void_p)
    assert L.sp_plan_execute_bursts(None, None, 0, 0, band, 1, one, one, 1, pc, None) == -1
    assert L.sp_power_bursts(None, None, 4, 0, band, 1, one, one, 1, pc, None) == -1
    assert L.sp_series_bursts(None, None, 1, 0, one, one, 1, pc, None) == -1
    assert L.sp_render_bursts(None, None, None, 0, 0, band, 1, one, one, 1, pc, None) == -1
    assert L.sp_plan_bursts_kernel_name_for(None, 0, 0) == b""
    v = np.array([0.0, 9.0, 9.0, 0.0])
    pv = v.ctypes.data_as(C.c_void_p)
    total = C.c_uint32(77)
    edges = np.full(5, 0x55555555, np.int32)
    pe = edges.ctypes.data
    dbg = L.sp_debug_bursts
    for hi, lo in ((math.nan, 1.0), (2.0, math.nan), (math.nan, math.nan), (1.0, 2.0), (0.0, 5e-324), (-3.0, 1.0)):   # NaN; lo > hi by key
        assert dbg(pv, 4, hi, lo, 2, C.byref(total), C.c_void_p(pe)) == -1, (hi, lo)
    assert dbg(pv, 4, 2.0, 1.0, 2, None, None) == -1                       # both outputs absent
    assert dbg(pv, 4, 2.0, 1.0, 0, None, C.c_void_p(pe)) == -1             # edges with max_bursts == 0 are absent
    assert dbg(pv, 4, 2.0, 1.0, -1, C.byref(total), C.c_void_p(pe)) == -1  # max_bursts < 0
    assert dbg(pv, 4, 2.0, 1.0, 2, C.byref(total), C.c_void_p(pe + 2)) == -1                     # misaligned edges
    assert dbg(pv, 4, 2.0, 1.0, 2, C.cast(C.c_void_p(C.addressof(cnt) + 1), C.POINTER(C.c_uint32)), C.c_void_p(pe)) == -1   # misaligned counts
    assert dbg(None, 4, 2.0, 1.0, 2, C.byref(total), C.c_void_p(pe)) == -1
    assert dbg(pv, -1, 2.0, 1.0, 2, C.byref(total), C.c_void_p(pe)) == -1
    assert total.value == 77 and (edges == 0x55555555).all()               # a refusal writes nothing
    # what is no refusal: lo == hi, a negative lo, both negative (key 0 both), -0.0, each output alone, no frames
    assert dbg(pv, 4, 2.0, 2.0, 2, C.byref(total), C.c_void_p(pe)) == 0 and total.value == 1 and edges.tolist()[:4] == [1, 3, -1, -1]
    assert edges[4] == 0x55555555
    assert dbg(pv, 4, 2.0, -1.0, 2, C.byref(total), None) == 0 and total.value == 1
    assert dbg(pv, 4, -2.0, -1.0, 1, None, C.c_void_p(pe)) == 0 and edges.tolist()[:2] == [0, 4]
    assert dbg(pv, 4, 0.0, -0.0, 0, C.byref(total), None) == 0 and total.value == 1
    assert dbg(None, 0, 2.0, 1.0, 2, C.byref(total), C.c_void_p(pe)) == 0 and total.value == 0 and edges.tolist()[:4] == [-1] * 4
    with pytest.raises(pkg.SpectroplotError) as e:
        pkg.burst_scan(v, 1.0, 2.0, 2)
    assert e.value.status == -1


def test_reference_on_hand_checked_series():
    nan, inf = math.nan, math.inf
    for row, hi, lo, want in (
            ([], 8, 2, []), ([9], 8, 2, [(0, 1)]), ([nan], 8, 2, []), ([1], 8, 2, []),
            ([0, 8, 5, 2, nan, 1.9, 8], 8, 2, [(1, 5), (6, 7)]),
            ([nan, 9, nan, 0, nan, 9], 8, 2, [(1, 3), (5, 6)]),
            ([9, 9, 0, 0, inf, 5], 8, 2, [(0, 2), (4, 6)]),
            ([1, 9, 1, 9, 1, 9], 8, 2, [(1, 2), (3, 4), (5, 6)]),
            ([5, 4.9, 5, nan, 4], 5, 5, [(0, 1), (2, 4)]),
            ([0, 9, 0, 0], 8, -1, [(1, 4)]),
            ([0.5, 5e-321, 1e-320, 2, 1e-320, 5e-324], 1.0, 1e-320, [(3, 5)])):
        assert burstref.scan(np.array(row, np.float64), hi, lo) == want, row
    counts, edges = burstref.expected(np.array([[1, 9, 1, 9, 1, 9.0], [0, 0, 0, 0, 0, 0]]), [8, 8], [2, 2], 2)
    assert counts.dtype == np.uint32 and counts.tolist() == [3, 0] and edges.dtype == np.int32
    assert edges.tolist() == [[[1, 2], [3, 4]], [[-1, -1], [-1, -1]]]


def test_planted_series_tell_at_every_shape_the_tests_use():
    """Asserted on the reference's output, not the library's: the expected bursts show every planted condition the shape has room
    for - at the GPU tests' shapes, and at the segment sizes of the stand-alone program."""
    S = _segment()
    everything = set()
    for seg in (64, 128, S):
        for seed in (0, 1):
            for count in (1, 3, 64):
                for width in gpu_widths(S)[:-1] + ((gpu_widths(S)[-1],) if (seg, seed) == (S, 0) else ()):
                    series, hi, lo = burstref.planted_series(seed, count, width, seg)
                    assert series.shape == (count, width)
                    got, need = burstref.telling(series, hi, lo, seg), burstref.must_tell(seed, count, width, seg)
                    assert need <= got, (seg, seed, count, width, sorted(need - got))
                    everything |= got
    assert len(everything) == 21, sorted(everything)
    # the widest shape holds every condition but the seed's other choice of a first frame; its alternating band is cut by max_bursts = 7
    wide = burstref.must_tell(0, 64, 64 * S + 5, S)
    assert len(wide) == 20 and "from_frame_0" not in wide
    counts, _ = burstref.planted_expected(0, 64, 2 * S + 3, S)
    assert counts[1] == (2 * S + 3) // 2 > 7 and counts[2] == 0


def _cases(S):
    """(series row, hi, lo, max_bursts): every band of planted series at small widths and 200 random series."""
    out = []
    for seed in (0, 1):
        for width in (1, 2, 63, 64, 65, 257, 2 * S + 3):
            series, hi, lo = burstref.planted_series(seed, 12, width, 64 if width < 2 * S else S)
            for b in range(12):
                for m in ((0, 1, 7, width // 2 + 1) if b < 6 and seed == 0 and width <= 257 else (7,)):
                    out.append((series[b], hi[b], lo[b], m))
    rng = np.random.default_rng(2027)
    vals = np.array([0.0, 1.0, 2.0, math.nextafter(2.0, 0), 5.0, 8.0, math.nextafter(8.0, 0), 9.0, math.inf, math.nan, -0.0, 5e-324])
    for i in range(200):
        width = int(rng.choice([0, 1, 5, 64, 130, 700]))
        row = rng.choice(vals, width, p=np.r_[np.full(4, 0.1), 0.3, np.full(7, 0.3 / 7)]) if i % 2 else rng.uniform(0, 10, width)
        hi, lo = ((8.0, 2.0), (5.0, 5.0), (8.0, -1.0), (math.inf, 2.0), (2.0, 0.0), (0.0, 0.0))[i % 6]
        out.append((row, hi, lo, int(rng.choice([0, 1, 3, width // 2 + 1]))))
    return out


def _want(row, hi, lo, m):
    bursts = burstref.scan(row, hi, lo)
    edges = np.full((m, 2), -1, np.int32)
    if m and bursts:
        edges[:min(m, len(bursts))] = bursts[:m]
    return len(bursts), edges


def test_debug_bursts_against_the_reference(pkg):
    checked = cut = none = 0
    for row, hi, lo, m in _cases(_segment()):
        total, edges = pkg.burst_scan(row, hi, lo, m)
        want_total, want_edges = _want(row, hi, lo, m)
        assert total == want_total and edges.dtype == np.int32 and np.array_equal(edges, want_edges), (len(row), hi, lo, m)
        checked += 1
        cut += total > m
        none += total == 0
    assert checked > 400 and cut > 50 and none > 20
    widths, gaps = pkg.burst_pulses([[1, 5], [6, 7], [10, 20], [-1, -1]], 3)
    assert widths.tolist() == [4, 1, 10] and gaps.tolist() == [1, 3]
    widths, gaps = pkg.burst_pulses(np.array([1, 5, 6, 7], np.int32), 9)          # a cut list: what is listed
    assert widths.tolist() == [4, 1] and gaps.tolist() == [1]
    assert [a.size for a in pkg.burst_pulses(np.zeros((0, 2)), 0)] == [0, 0]


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/sp_burst_core.h alone, host compiler, -fsanitize=address,undefined: the same series through stdin, scanned by the host
    loop and as the kernels scan (words, summaries per segment of 64, 128 and SP_BURST_SEGMENT_FRAMES frames, the exclusive combine
    scan, the emit with popcounts and one writer per slot), combine's associativity on all triples of small summaries first; the
    answers against burstref."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "burst_core_check")
    csrc = os.path.join(ROOT, "spectroplot-js_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # (the runtimes linked in)
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "burst_core_check.cpp")])
    S = _segment()
    cases = _cases(S)
    series, hi, lo = burstref.planted_series(0, 6, 5 * S + 70, S)       # the segment edges and the three-segment burst at the real size
    cases += [(series[b], hi[b], lo[b], 7) for b in range(6)]
    series, hi, lo = burstref.planted_series(1, 2, 64 * 128 + 5, 128)   # a second step of the carry scan at segments of 128 and 64
    cases += [(series[b], hi[b], lo[b], 5000) for b in range(2)]
    bits = lambda v: "%016x" % np.array([v], np.float64).view(np.uint64)[0]  # noqa: E731
    lines, want = [], []
    for row, h, l, m in cases:
        row = np.ascontiguousarray(row, np.float64)
        lines.append("%s %s %d %d %s" % (bits(h), bits(l), m, len(row), " ".join("%x" % b for b in row.view(np.uint64).tolist())))
        total, edges = _want(row, h, l, m)
        want.append(" ".join(str(v) for v in [total] + edges.reshape(-1).tolist()))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(want) + 1 and got[-1] == ""
    for line, g, w in zip(lines, got, want):
        assert g == w, (line[:80], g[:200], w[:200])
