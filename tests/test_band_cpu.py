"""The exact band-power series without a device: the ABI, and sp_band_rows - the rows of a frequency range - against tests/bandref.py
for every n from 2 to 4096, against a hand-checked table, and through a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/cpp/band_rows_check.cpp)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bandref
import meanref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_band_rows", "sp_power_bands", "sp_plan_execute_bandpower", "sp_render_bandpower", "sp_plan_bandpower_kernel_name_for")
INF = math.inf


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    flat = " ".join(hdr.split())
    for decl in ("#define SP_MAX_BANDS 64",
                 "int sp_band_rows(int32_t n, double f_lo, double f_hi, int32_t *y0, int32_t *y1);",
                 "int sp_power_bands(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, "
                 "double *d_band);",
                 "int sp_plan_execute_bandpower(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, "
                 "int32_t count, double *d_band);",
                 "int sp_render_bandpower(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, "
                 "const int32_t *bands, int32_t count, int32_t db, double *band);",
                 "const char *sp_plan_bandpower_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);"):
        assert decl in flat, decl
    text = hdr[hdr.index("Exact band-power series"):hdr.index("#define SP_MAX_BANDS")]
    for word in ("SP_ERR_UNSUPPORTED", "SP_ERR_INVALID_ARG", "SP_ERR_NOT_POW2", "NaN", "math.fsum", "2^1024 - 2^970", "BAND-MAJOR", "HOST array",
                 "+0.0", "SUM, not a mean", "NOR ON THE CU COUNT", "sp_plan_power_to_db", "I/Q plans", "Out of scope", "weighted bands",
                 "sharding.py", "fused into"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_bandpower", "bandpower_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_bandpower", "power_bands"):
        assert hasattr(pkg.Context, name), name
    assert callable(pkg.binding.band_rows) and callable(pkg.band_rows) and pkg.binding.SP_MAX_BANDS == bandref.SP_MAX_BANDS == 64
    # no existing structure changed
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.DETECTORS == {"sample": 0, "peak": 1}


def test_null_handles_are_invalid_arguments(pkg):
    L = pkg.Library.get().L
    bands = (C.c_int32 * 2)(0, 1)
    assert L.sp_power_bands(None, None, 4, 0, bands, 1, None) == -1
    assert L.sp_plan_execute_bandpower(None, None, 0, 0, bands, 1, None) == -1
    assert L.sp_render_bandpower(None, None, None, 0, 0, bands, 1, 0, None) == -1
    assert L.sp_plan_bandpower_kernel_name_for(None, 0, 0) == b""
    y0, y1 = C.c_int32(7), C.c_int32(7)
    assert L.sp_band_rows(8, 0.0, 0.0, None, C.byref(y1)) == -1
    assert L.sp_band_rows(8, 0.0, 0.0, C.byref(y0), None) == -1
    assert (y0.value, y1.value) == (7, 7)


def _edges(n):
    """Edges in cycles per sample: exact bin centres, half-way points, +-1/2, values beyond them, tiny offsets and infinities."""
    centres = [k / n for k in (-n // 2, -n // 2 + 1, -1, 0, 1, n // 2 - 1, n // 2)]
    out = set(centres)
    for c in centres:
        out.update((c + 0.5 / n, c - 0.5 / n, math.nextafter(c, INF), math.nextafter(c, -INF)))
    out.update((-0.5, 0.5, -0.75, 0.75, -3.0, 3.0, 0.1, -0.1, 1 / 3, -INF, INF))
    return sorted(out)


def test_band_rows_against_the_formula_for_every_n(pkg):
    """Every n from 2 to 4096: the powers of two over the grid of edges, every other n refused."""
    L = pkg.Library.get().L
    y0, y1 = C.c_int32(), C.c_int32()
    empty = full = checked = 0
    for n in range(2, 4097):
        if n & (n - 1):
            assert L.sp_band_rows(n, -0.25, 0.25, C.byref(y0), C.byref(y1)) == -2, n
            continue
        edges = _edges(n)
        for i, lo in enumerate(edges):
            for hi in edges[i:]:
                assert L.sp_band_rows(n, lo, hi, C.byref(y0), C.byref(y1)) == 0, (n, lo, hi)
                want = bandref.band_rows(n, lo, hi)
                assert (y0.value, y1.value) == want, (n, lo, hi, (y0.value, y1.value), want)
                assert 0 <= want[0] <= want[1] <= n
                empty += want[0] == want[1]
                full += want == (0, n)
                checked += 1
    assert checked > 5000 and empty > 100 and full > 100


def test_band_rows_hand_checked_table(pkg):
    """n = 8: f(y) = .5, .375, .25, .125, 0, -.125, -.25, -.375 for y = 0 .. 7."""
    f = [(4 - y) / 8 for y in range(8)]
    assert f == [.5, .375, .25, .125, 0, -.125, -.25, -.375]
    table = [((0.0, 0.0), (4, 5)), ((-0.5, 0.5), (0, 8)), ((-1.0, 1.0), (0, 8)), ((0.125, 0.375), (1, 4)), ((0.1, 0.4), (1, 4)),
             ((0.126, 0.374), (2, 3)), ((0.13, 0.2), (3, 3)), ((-0.375, -0.375), (7, 8)), ((-0.5, -0.4), (8, 8)), ((0.5, 0.5), (0, 1)),
             ((0.51, 0.9), (0, 0)), ((-0.125, 0.125), (3, 6)), ((-INF, 0.0), (4, 8)), ((0.0, INF), (0, 5)), ((-9.0, -0.6), (8, 8))]
    for (lo, hi), want in table:
        assert pkg.band_rows(8, lo, hi) == want == bandref.band_rows(8, lo, hi), (lo, hi)
        rows = [y for y in range(8) if lo <= f[y] <= hi]
        assert list(range(*want)) == rows, (lo, hi)
    assert pkg.band_rows(2, -0.5, 0.5) == (0, 2) and pkg.band_rows(2, 0.0, 0.0) == (1, 2) and pkg.band_rows(1 << 20, 0.0, 0.0) == (1 << 19, (1 << 19) + 1)


def test_band_rows_refusals(pkg):
    for n, lo, hi, status in ((8, math.nan, 0.0, -1), (8, 0.0, math.nan, -1), (8, 0.25, 0.125, -1), (8, INF, -INF, -1), (1, 0.0, 0.0, -1),
                              (0, 0.0, 0.0, -1), (-8, 0.0, 0.0, -1), (3, 0.0, 0.0, -2), (12, 0.0, 0.0, -2), (4095, 0.0, 0.0, -2)):
        with pytest.raises(pkg.SpectroplotError) as e:
            pkg.band_rows(n, lo, hi)
        assert e.value.status == status, (n, lo, hi)


def test_reference_band_sums_of_a_plane():
    tiny, big = 5e-324, np.finfo(np.float64).max
    plane = np.array([[1.0, 2.0, 4.0, 8.0],
                      [2.0 ** 53, 1.0, tiny, 0.0],
                      [big, big, 0.0, 1.0],
                      [1.0, math.nan, math.inf, 2.0]])
    got = bandref.expected(plane, [(0, 4), (0, 0), (1, 2), (2, 4), (0, 2)])
    want = np.array([[15.0, 2.0 ** 53 + 2, INF, math.nan], [0.0] * 4, [2.0, 1.0, big, math.nan], [12.0, tiny, 1.0, INF],
                     [3.0, 2.0 ** 53, INF, math.nan]])
    assert meanref.same(got, want) and got.shape == (5, 4)
    assert (got[1].view(np.uint64) == 0).all()                                   # +0.0
    assert meanref.same(got[2], plane[:, 1])                                     # a band of one row is the plane's column
    assert bandref.expected(np.zeros((0, 4)), [(0, 4)]).shape == (1, 0) and bandref.expected(plane, []).shape == (0, 4)
    # the synthetic planes of the GPU test hold what they are meant to hold: every kind of frame, and frame 5 overflows
    p = bandref.synthetic_plane(1, 64, 13)
    assert p.shape == (13, 64) and (p >= 0).all() and np.isfinite(p).all() and (p[2] < 2.0 ** -1022).all()
    e = p[0].view(np.uint64) >> np.uint64(52)
    assert e.max() - e.min() > 1500
    assert np.isinf(bandref.expected(p, [(0, 64)])[0, 5]) and bandref.expected(p, [(0, 1)])[0, 5] == big
    assert bandref.standard_bands(2) == [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2), (1, 2), (0, 2), (0, 2)]
    assert bandref.standard_bands(100)[3:5] == [(1, 64), (3, 68)]


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/sp_geometry.cpp's band code, host compiler, -fsanitize=address,undefined: rows of frequency ranges and band lists through
    stdin, the answers against bandref."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "band_rows_check")
    csrc = os.path.join(ROOT, "spectroplot-js_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # (the runtimes linked in)
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "band_rows_check.cpp"), os.path.join(csrc, "sp_geometry.cpp")])
    lines, want = [], []
    for n in (2, 8, 64, 4096, 1 << 20):
        edges = _edges(n)
        for i, lo in enumerate(edges):
            for hi in edges[i::3]:
                lines.append("rows %d %s %s" % (n, float(lo).hex(), float(hi).hex()))
                want.append("0 %d %d" % bandref.band_rows(n, lo, hi))
    for n, lo, hi, status in ((8, math.nan, 0.0, -1), (8, 0.25, 0.125, -1), (1, 0.0, 0.0, -1), (12, 0.0, 0.0, -2)):
        lines.append("rows %d %s %s" % (n, float(lo).hex(), float(hi).hex()))
        want.append("%d" % status)
    for n, bands, ok in ((8, [], True), (8, [0, 0, 0, 8, 8, 8, 3, 5], True), (8, [0, 9], False), (8, [-1, 2], False), (8, [5, 4], False),
                         (8, [0, 1] * 64, True), (8, [0, 1] * 65, False)):
        lines.append("bands %d %d %s" % (n, len(bands) // 2, " ".join(map(str, bands))))
        want.append("ok" if ok else "refused")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(want) + 1 and got[-1] == ""
    for line, g, w in zip(lines, got, want):
        assert g == w, (line, g, w)
