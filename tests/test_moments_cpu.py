"""The exact spectral moments without a device: the ABI and its refusals, tests/momentref.py against hand-checked values, and
sp_debug_moment_sum - the host side of the code the moment kernel runs - bit for bit against momentref, directly and through a
stand-alone program built with the address and undefined-behaviour sanitizers (tests/cpp/moment_core_check.cpp)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import meanref
import momentref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_power_moments", "sp_plan_execute_moments", "sp_render_moments", "sp_debug_moment_sum", "sp_plan_moments_kernel_name_for")
INF = math.inf
BIG, TINY = float(np.finfo(np.float64).max), 5e-324


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    flat = " ".join(hdr.split())
    for decl in ("int sp_power_moments(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, "
                 "int32_t order, double *d_out);",
                 "int sp_plan_execute_moments(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, "
                 "int32_t count, int32_t order, double *d_out);",
                 "int sp_render_moments(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, "
                 "const int32_t *bands, int32_t count, int32_t order, int32_t db, double *out);",
                 "int sp_debug_moment_sum(const double *values, size_t count, int32_t order, double *out);",
                 "const char *sp_plan_moments_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);"):
        assert decl in flat, decl
    text = hdr[hdr.index("Exact spectral moments"):hdr.index("int sp_power_moments(")]
    for word in ("MOMENT-MAJOR", "(y - y0_b)^k", "0^0 = 1", "2^1024 - 2^970", "THE BAND'S, NOT THE TERM'S", "0 * inf", "+0.0", "m[0] ONLY",
                 "no dB form", "SP_ERR_UNSUPPORTED", "SP_ERR_INVALID_ARG", "NOR ON THE CU COUNT", "bit for bit", "Out of scope"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_moments", "moments_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_moments", "power_moments"):
        assert hasattr(pkg.Context, name), name
    assert callable(pkg.moment_sum) and callable(pkg.centroid_freq) and pkg.binding.moment_sum is pkg.moment_sum
    assert "moment_sum" in pkg.__all__ and "centroid_freq" in pkg.__all__
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56      # no existing structure changed


def test_bad_arguments_are_refused_without_a_device(pkg):
    L = pkg.Library.get().L
    bands = (C.c_int32 * 2)(0, 1)
    for order in (-1, 0, 1, 2, 3):
        assert L.sp_power_moments(None, None, 4, 0, bands, 1, order, None) == -1
        assert L.sp_plan_execute_moments(None, None, 0, 0, bands, 1, order, None) == -1
        assert L.sp_render_moments(None, None, None, 0, 0, bands, 1, order, 0, None) == -1
    assert L.sp_plan_moments_kernel_name_for(None, 0, 0) == b""
    # the debug entry: orders, null outputs, negative values, a column past SP_MAX_N rows
    v = np.array([1.0, 2.0, 3.0])
    out = np.full(4, 7.0)
    vp = C.c_void_p
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    for order in (-1, 3, 1 << 20):
        assert L.sp_debug_moment_sum(p(v), 3, order, p(out)) == -1
    assert L.sp_debug_moment_sum(p(v), 3, 2, None) == -1
    assert L.sp_debug_moment_sum(None, 3, 2, p(out)) == -1
    for bad in (-1.0, -0.0, -INF, -TINY):
        assert L.sp_debug_moment_sum(p(np.array([1.0, bad])), 2, 2, p(out)) == -1
    long = np.zeros((1 << 20) + 1)
    assert L.sp_debug_moment_sum(p(long), long.size, 0, p(out)) == -1
    assert (out == 7.0).all()                                           # a refusal writes nothing
    assert L.sp_debug_moment_sum(p(v), 3, 1, p(out)) == 0 and list(out) == [6.0, 8.0, 7.0, 7.0]   # order + 1 values and no more
    assert L.sp_debug_moment_sum(None, 0, 2, p(out)) == 0 and (out[:3].view(np.uint64) == 0).all()  # the empty sum: +0.0
    with pytest.raises(pkg.SpectroplotError):
        pkg.moment_sum([1.0], order=3)
    # a negative NaN is a NaN
    assert np.isnan(pkg.moment_sum([1.0, -math.nan, 2.0])).all()


def test_reference_against_hand_checked_values():
    rng = np.random.default_rng(5)
    for clustered in (False, True):
        v = meanref.random_values(rng, 200, clustered)
        assert momentref.weighted_sum(v, 0) == meanref.exact_sum(v) == math.fsum(v)      # k = 0 is math.fsum
    assert momentref.weighted_sum([3.0, 2.0 ** 53 + 2, 0.5], 1) == 2.0 ** 53 + 4         # 2^53 + 3: a tie, to even (up)
    assert momentref.weighted_sum([3.0, 2.0 ** 53, 0.5], 1) == 2.0 ** 53                 # 2^53 + 1: a tie, to even (down)
    got = momentref.column([0.0, 0.0, BIG])
    assert got[0] == BIG and got[1] == INF and got[2] == INF                             # DBL_MAX at weight 2, and m0 stays finite
    assert momentref.column([0.0, BIG])[1] == BIG and momentref.column([BIG, 1.0, 2.0])[2] == 9.0
    assert momentref.weighted_sum([0.0] * 1024 + [TINY], 1) == 1024 * TINY
    assert momentref.weighted_sum([0.0] * 1024 + [TINY], 2) == 1024 * 1024 * TINY
    # special values are the band's: row 0 has weight 0, and still marks every moment
    assert np.isinf(momentref.column([INF, 1.0, 2.0])).all() and np.isnan(momentref.column([math.nan, 1.0])).all()
    assert np.isnan(momentref.column([INF, 1.0, math.nan])).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.float64(0.0) * np.float64(INF))                               # ... which numpy's product would not
    assert (momentref.column([]).view(np.uint64) == 0).all()
    one = momentref.column([3.5])
    assert one[0] == 3.5 and (one[1:].view(np.uint64) == 0).all()                        # one row: m1 = m2 = +0.0
    plane = np.array([[1.0, 2.0, 4.0, 8.0], [2.0 ** 53, 1.0, TINY, 0.0]])
    want = momentref.expected(plane, [(0, 4), (1, 3), (2, 2)])
    assert want.shape == (3, 3, 2) and list(want[:, 0, 0]) == [15.0, 34.0, 90.0] and list(want[:, 1, 0]) == [6.0, 4.0, 4.0]
    assert (want[:, 2].view(np.uint64) == 0).all()
    small = np.array([0.0, 3.0, 0.0, 5.0])
    assert meanref.same(momentref.last_row_expected(small), momentref.column(small))
    # the integer form the GPU test uses for its column of 2^20 rows is the same reference
    for name, values in momentref.columns():
        assert meanref.same(momentref.dense_column(values), momentref.column(values)), name


def test_debug_moment_sum_is_the_reference_bit_for_bit(pkg):
    names = set()
    for name, values in momentref.columns():
        names.add(name)
        want = momentref.column(values)
        meanref.assert_same(pkg.moment_sum(values, 2), want, name)
        for order in (0, 1):
            meanref.assert_same(pkg.moment_sum(values, order), want[:order + 1], "%s, order %d" % (name, order))
        if not np.isnan(want[0]):
            assert pkg.moment_sum(values, 0)[0] == pkg.binding.exact_sum(values), name     # m0 is the exact sum
    assert {"full range", "denormals", "tie to even, up", "tie to even, down", "DBL_MAX at weight 2", "nan in row 0", "inf in row 0",
            "cell 63 shift 12", "cell 0 shift 0", "cell 62 shift 31", "cell 1 shift 11"} <= names
    assert list(pkg.moment_sum([0.0, 0.0, BIG])) == [BIG, INF, INF] and list(pkg.moment_sum([0.0, BIG], 1)) == [BIG, BIG]
    assert pkg.moment_sum([3.0, 2.0 ** 53 + 2, 0.5])[1] == 2.0 ** 53 + 4 and pkg.moment_sum([3.0, 2.0 ** 53, 0.5])[1] == 2.0 ** 53


def test_debug_moment_sum_at_the_largest_weight(pkg):
    """2^20 rows with the value in the last one: the weight (2^20 - 1)^2, the largest a band can give."""
    values = momentref.last_row_column()
    assert values.size == 1 << 20 and values[-1] > 0 and not values[:-1].any()
    meanref.assert_same(pkg.moment_sum(values, 2), momentref.last_row_expected(values), "the last of 2^20 rows")
    values[-1] = BIG
    want = momentref.last_row_expected(values)
    assert list(want) == [BIG, INF, INF]
    meanref.assert_same(pkg.moment_sum(values, 2), want, "DBL_MAX in the last of 2^20 rows")
    # every row set: 2^20 pieces in one cell, the cell bound of csrc/sp_moment_core.h
    full = np.full(1 << 20, np.array([(1000 << 52) | 0x000fffffffffffff], np.uint64).view(np.float64)[0])
    rows, v = 1 << 20, Fraction(float(full[0]))
    want = np.array([float(v * rows), float(v * (rows * (rows - 1) // 2)), float(v * ((rows - 1) * rows * (2 * rows - 1) // 6))])
    meanref.assert_same(pkg.moment_sum(full, 2), want, "2^20 equal rows")


def _hex(values):
    return " ".join("%x" % b for b in np.ascontiguousarray(values, np.float64).view(np.uint64))


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/sp_moment_core.h over csrc/sp_exact_sum.h, host compiler, -fsanitize=address,undefined: the columns through stdin, the
    bits against momentref.  The program also puts every value's pieces back together against the 128-bit product."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "moment_core_check")
    csrc = os.path.join(ROOT, "spectroplot-js_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # (the runtimes linked in)
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "moment_core_check.cpp")])
    lines, want, names = [], [], []
    for name, values in momentref.columns():
        for order in (2, 1, 0) if name in ("full range", "tie to even, up") else (2,):
            lines.append("column %d %d %s" % (order, values.size, _hex(values)))
            want.append(momentref.column(values, order))
            names.append(name)
    last = momentref.last_row_column()
    lines.append("sparse 2 %d %d %s" % (last.size, last.size - 1, _hex(last[-1:])))
    want.append(momentref.last_row_expected(last))
    names.append("the last of 2^20 rows")
    refused = ["column 3 1 %s" % _hex([1.0]), "column -1 1 %s" % _hex([1.0]), "column 2 2 %s" % _hex([1.0, -1.0]),
               "sparse 0 %d 0 %s" % ((1 << 20) + 1, _hex([1.0]))]
    run = subprocess.run([exe], input="\n".join(lines + refused) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(lines) + len(refused) + 1 and got[-1] == ""
    for name, g, w in zip(names, got, want):
        bits = np.array([int(t, 16) for t in g.split()], np.uint64)
        meanref.assert_same(bits.view(np.float64), w, name)
    assert got[len(lines):-1] == ["refused"] * len(refused)
