"""The peak track without a device: the ABI, and the one comparison of csrc/sp_track_core.h against tests/trackref.py - numpy's argmax
over the values that are not NaN - bit for bit, through the library's host side (sp_debug_band_peak) and through a stand-alone program
built with the address and undefined-behaviour sanitizers (tests/cpp/track_core_check.cpp); row_freq against bandref.band_rows."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bandref
import trackref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_power_tracks", "sp_plan_execute_track", "sp_render_track", "sp_plan_track_kernel_name_for", "sp_debug_band_peak")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    flat = " ".join(hdr.split())
    for decl in ("int sp_power_tracks(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, "
                 "int32_t *d_row, double *d_peak);",
                 "int sp_plan_execute_track(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, "
                 "int32_t count, int32_t *d_row, double *d_peak);",
                 "int sp_render_track(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, "
                 "const int32_t *bands, int32_t count, int32_t db, int32_t *row, double *peak);",
                 "const char *sp_plan_track_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);",
                 "int sp_debug_band_peak(const double *values, int32_t n, int32_t y0, int32_t y1, int32_t *row, double *peak);"):
        assert decl in flat, decl
    text = hdr[hdr.index("Peak track:"):hdr.index("int sp_power_tracks(")]
    for word in ("SP_ERR_UNSUPPORTED", "SP_ERR_INVALID_ARG", "A NaN IS ANY NaN", "BAND-MAJOR", "HOST array", "THE SMALLEST y WINS", "+0.0",
                 "row = -1", "argmax", "NOR ON THE CU COUNT", "sp_plan_power_to_db", "worker.js:85-92", "0x7ff0000000000000", "4-byte",
                 "8-byte", "Out of scope", "sharding.py", "fused into", "sub-bin interpolation", "threshold", "more than one peak"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_track", "track_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_track", "power_tracks"):
        assert hasattr(pkg.Context, name), name
    assert callable(pkg.binding.band_peak) and callable(pkg.band_peak) and callable(pkg.binding.row_freq) and callable(pkg.row_freq)
    # no existing structure changed
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.DETECTORS == {"sample": 0, "peak": 1} and b.SP_MAX_BANDS == 64


def test_null_handles_and_refusals_of_the_debug_entry(pkg):
    L = pkg.Library.get().L
    bands = (C.c_int32 * 2)(0, 1)
    assert L.sp_power_tracks(None, None, 4, 0, bands, 1, None, None) == -1
    assert L.sp_plan_execute_track(None, None, 0, 0, bands, 1, None, None) == -1
    assert L.sp_render_track(None, None, None, 0, 0, bands, 1, 0, None, None) == -1
    assert L.sp_plan_track_kernel_name_for(None, 0, 0) == b""
    v = np.array([1.0, 3.0, 2.0, 3.0])
    p = v.ctypes.data_as(C.c_void_p)
    row, peak = C.c_int32(77), C.c_double(77.0)
    dbg = L.sp_debug_band_peak
    for n, y0, y1 in ((4, -1, 2), (4, 3, 2), (4, 0, 5), (4, 5, 5), (0, 0, 0), (-4, 0, 0)):                       # a bad band, a bad n
        assert dbg(p, n, y0, y1, C.byref(row), C.byref(peak)) == -1, (n, y0, y1)
    assert dbg(p, 4, 0, 4, None, None) == -1                                                                   # both outputs NULL
    assert dbg(None, 4, 0, 4, C.byref(row), C.byref(peak)) == -1
    assert (row.value, peak.value) == (77, 77.0)
    assert dbg(p, 4, 0, 4, C.byref(row), None) == 0 and row.value == 1                                         # either one may be NULL
    assert dbg(p, 4, 2, 4, None, C.byref(peak)) == 0 and peak.value == 3.0
    assert dbg(p, 4, 2, 2, C.byref(row), C.byref(peak)) == 0 and row.value == -1 and math.isnan(peak.value)    # an empty band
    with pytest.raises(pkg.SpectroplotError) as e:
        pkg.band_peak(v, 2, 1)
    assert e.value.status == -1


def _same(got, want):
    return got[0] == want[0] and (math.isnan(got[1]) and math.isnan(want[1]) or
                                  np.float64(got[1]).view(np.uint64) == np.float64(want[1]).view(np.uint64))


def test_reference_on_a_hand_checked_plane():
    nan, inf, tiny = math.nan, math.inf, 5e-324
    plane = np.array([[1.0, 4.0, 4.0, 2.0],
                      [0.0, 0.0, 0.0, 0.0],
                      [nan, tiny, 0.0, nan],
                      [nan, nan, nan, nan],
                      [1.0, inf, nan, inf]])
    rows, peaks = trackref.expected(plane, [(0, 4), (0, 0), (2, 4), (0, 1), (3, 4)])
    assert rows.dtype == np.int32 and rows.tolist() == [[1, 0, 1, -1, 1], [-1] * 5, [2, 2, 2, -1, 3], [0, 0, -1, -1, 0], [3, 3, -1, -1, 3]]
    want = np.array([[4.0, 0.0, tiny, nan, inf], [nan] * 5, [4.0, 0.0, 0.0, nan, inf], [1.0, 0.0, nan, nan, 1.0], [2.0, 0.0, nan, nan, inf]])
    bandref.assert_same(peaks, want, "hand-checked")
    assert trackref.expected(np.zeros((0, 4)), [(0, 4)])[0].shape == (1, 0) and trackref.expected(plane, [])[1].shape == (0, 5)
    for x in range(5):
        assert _same(trackref.frame_peak(plane[x, 0:4], 0), (rows[0, x], peaks[0, x]))
    # the synthetic plane holds what it is meant to hold
    n, width = 100, 65
    p = trackref.synthetic_plane(3, n, width)
    assert p.shape == (width, n) and not (np.signbit(p) & ~np.isnan(p)).any()
    r, k = trackref.expected(p, [(0, n), (1, 64), (6, 70), (64, n)])
    assert r[0, :6].tolist() == [5, 5, 8, 0, 0, 0] and k[0, :6].tolist() == [2.0, 2.0, 2.0, 1.5, 0.0, 2.0]
    assert r[2, 1] == 69 and r[2, 2] == 8 and r[3, 5] == n - 1
    q0, q1 = n // 3, n - 1 - n // 5
    assert r[0, 6:11].tolist() == [q1, q0, q1, q0, q1]
    assert k[0, 6:11].view(np.uint64).tolist() == [large for _, large in trackref.PAIRS]
    assert np.isnan(p[11:14, n // 2]).all() and (r[0, 11:14] != n // 2).all() and (r[0, 11:14] >= 0).all()
    assert r[1, 14] == -1 and np.isnan(k[1, 14]) and r[0, 14] in (0, *range(64, n))
    assert r[0, 15] == n // 2 == r[0, 16] and np.isinf(k[0, 15]) and np.isinf(k[0, 16])
    b = p.view(np.uint64)
    assert b[12, n // 2] == trackref.NEGATIVE_NAN and b[13, n // 2] == trackref.SIGNALLING_NAN > b[13, :n // 2].max()


def test_band_peak_against_the_reference(pkg):
    """sp_debug_band_peak - the host side of the code the kernel runs - on every frame of a synthetic plane for the standard bands, and
    on a few thousand random lists."""
    checked = ties = nans = empty = 0
    for n in (2, 64, 100, 256):
        plane = trackref.synthetic_plane(11 * n, n, 40)
        bands = bandref.standard_bands(n) + [(min(2, n), n)]
        rows, peaks = trackref.expected(plane, bands)
        for x in range(plane.shape[0]):
            for b, (y0, y1) in enumerate(bands):
                got = pkg.band_peak(plane[x], y0, y1)
                assert _same(got, (rows[b, x], peaks[b, x])), (n, x, y0, y1, got, rows[b, x], peaks[b, x])
                checked += 1
    for v, y0, y1 in trackref.random_lists(2024, 3000):
        want = trackref.frame_peak(v[y0:y1], y0)
        got = pkg.band_peak(v, y0, y1)
        assert _same(got, want), (v, y0, y1, got, want)
        p = v[y0:y1]
        empty += want[0] < 0
        nans += bool(np.isnan(p).any())
        ties += want[0] >= 0 and int((p == want[1]).sum()) > 1
        checked += 1
    assert checked > 4000 and ties > 300 and nans > 500 and empty > 100


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/sp_track_core.h alone, host compiler, -fsanitize=address,undefined: the planted frames and the random lists through stdin,
    folded ascending and as the wave folds them; the answers against trackref."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "track_core_check")
    csrc = os.path.join(ROOT, "spectroplot-js_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # (the runtimes linked in)
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "track_core_check.cpp")])
    frames = []
    for n in (2, 64, 100, 256):
        plane = trackref.synthetic_plane(11 * n, n, 40)
        for x in range(plane.shape[0]):
            for y0, y1 in bandref.standard_bands(n) + [(min(2, n), n)]:
                frames.append((plane[x], y0, y1))
    frames += trackref.random_lists(2024, 3000)
    lines, want = [], []
    for v, y0, y1 in frames:
        lines.append("%d %d %d %s" % (y0, y1, len(v), " ".join("%016x" % b for b in np.ascontiguousarray(v).view(np.uint64).tolist())))
        row, peak = trackref.frame_peak(v[y0:y1], y0)
        want.append((row, None if row < 0 else int(np.float64(peak).view(np.uint64))))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(want) + 1 and got[-1] == ""
    for line, g, (row, bits) in zip(lines, got, want):
        r, b = g.split(" ")
        assert int(r) == row, (line[:80], g, row)
        if row < 0:
            assert int(b, 16) & 0x7fffffffffffffff > 0x7ff0000000000000, (line[:80], g)      # any NaN
        else:
            assert int(b, 16) == bits, (line[:80], g, "%016x" % bits)


def test_row_freq_is_the_inverse_of_band_rows(pkg):
    for n in (2, 64, 1024):
        for y in range(n):
            f = pkg.row_freq(n, y)
            assert f == (n // 2 - y) / n
            assert bandref.band_rows(n, f, f) == (y, y + 1) == pkg.band_rows(n, f, f), (n, y)
    assert pkg.row_freq(8, 0) == 0.5 and pkg.row_freq(8, 4) == 0.0 and pkg.row_freq(8, 7) == -0.375
    assert math.isnan(pkg.row_freq(64, -1))
    assert "I/Q plans" in pkg.binding.row_freq.__doc__
