"""The exact variance sums without a device: the ABI and its refusals, tests/varianceref.py against hand-checked values,
sp_debug_variance_sums - the host side of the code the variance kernels run - bit for bit against varianceref, directly and through a
stand-alone program built with the address and undefined-behaviour sanitizers (tests/cpp/variance_core_check.cpp), and the launch rule
of the accumulation restated."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import meanref
import varianceref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_power_variance", "sp_plan_execute_variance", "sp_render_variance", "sp_debug_variance_sums", "sp_debug_variance_launch",
                "sp_plan_variance_kernel_name_for")
INF = math.inf
BIG, TINY = float(np.finfo(np.float64).max), 5e-324


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    flat = " ".join(hdr.split())
    for decl in ("int sp_power_variance(sp_context *ctx, const double *d_power, int32_t n, int32_t width, double *d_out);",
                 "int sp_plan_execute_variance(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_out);",
                 "int sp_render_variance(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, "
                 "double *out);",
                 "int sp_debug_variance_sums(const double *values, size_t count, double *out3);",
                 "int sp_debug_variance_launch(int32_t n, int64_t frames, int32_t cu_count, int64_t *out, size_t capacity, size_t *used);",
                 "const char *sp_plan_variance_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);"):
        assert decl in flat, decl
    text = hdr[hdr.index("Exact variance and spectral-kurtosis traces"):hdr.index("int sp_power_variance(")]
    for word in ("double[3 * n]", "W * S2 - S1^2", "106-bit", "Cauchy-Schwarz", "DENORMAL RANGE", "2^-2148", "+0.0", "A NaN IS ANY NaN",
                 "no dB form", "SP_ERR_UNSUPPORTED", "SP_ERR_INVALID_ARG", "NOR ON THE CU COUNT", "bit for bit", "lib/worker.js", "Out of scope"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_variance", "variance_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_variance", "power_variance"):
        assert hasattr(pkg.Context, name), name
    for name in ("variance_sums", "variance_of", "spectral_kurtosis"):
        assert callable(getattr(pkg, name)) and getattr(pkg.binding, name) is getattr(pkg, name) and name in pkg.__all__, name
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56      # no existing structure changed


def test_bad_arguments_are_refused_without_a_device(pkg):
    L = pkg.Library.get().L
    assert L.sp_power_variance(None, None, 4, 0, None) == -1
    assert L.sp_plan_execute_variance(None, None, 0, 0, None) == -1
    assert L.sp_render_variance(None, None, None, 0, 0, None) == -1
    assert L.sp_plan_variance_kernel_name_for(None, 0, 0) == b""
    v = np.array([1.0, 2.0, 3.0])
    out = np.full(4, 7.0)
    vp = C.c_void_p
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    assert L.sp_debug_variance_sums(p(v), 3, None) == -1
    assert L.sp_debug_variance_sums(None, 3, p(out)) == -1
    for bad in (-1.0, -0.0, -INF, -TINY):
        assert L.sp_debug_variance_sums(p(np.array([1.0, bad])), 2, p(out)) == -1
    assert L.sp_debug_variance_sums(p(v), 1 << 31, p(out)) == -1        # (refused before a value is read)
    assert (out == 7.0).all()                                           # a refusal writes nothing
    assert L.sp_debug_variance_sums(p(v), 3, p(out)) == 0 and list(out) == [6.0, 14.0, 6.0, 7.0]   # three values and no more
    assert L.sp_debug_variance_sums(None, 0, p(out)) == 0 and (_bits(out[:3]) == 0).all()          # the sums of nothing: +0.0
    assert np.isnan(pkg.variance_sums([1.0, -math.nan, 2.0])).all()     # a negative NaN is a NaN
    used = C.c_size_t()
    grid = np.zeros(3, np.int64)
    for n, frames, cu in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.sp_debug_variance_launch(n, frames, cu, p(grid), 3, C.byref(used)) == -1
    assert L.sp_debug_variance_launch(64, 64, 8, p(grid), 2, C.byref(used)) == -1 and used.value == 3
    assert L.sp_debug_variance_launch(64, 64, 8, p(grid), 3, None) == -1 and not grid.any()


def test_reference_against_hand_checked_values():
    col = varianceref.column
    assert list(col([1.0, 1.0, 1.0])) == [3.0, 3.0, 0.0] and _bits(col([1.0, 1.0, 1.0]))[2] == 0
    assert list(col([1.0, 2.0, 3.0])) == [6.0, 14.0, 6.0]
    got = col([2.0 ** -537] * 2)
    assert got[0] == 2.0 ** -536 and got[1] == 2.0 ** -1073 and _bits(got)[1] == 2 and got[2] == 0.0
    # float() of a Fraction rounds correctly into the denormal range
    from fractions import Fraction
    assert float(Fraction(5e-324) * Fraction(3, 2)) == 1e-323
    # ties in the denormal grid: 2^-1074 + 2^-1076 lies below the half step, 1.5 * 2^-1074 ties to the even 2 * 2^-1074,
    # 2.5 ties to the even 2, 3.25 rounds down to 3, and a square of a quarter of a denormal rounds to zero
    assert _bits(col([2.0 ** -537, 2.0 ** -538]))[1] == 1
    assert _bits(col([2.0 ** -537, 2.0 ** -538, 2.0 ** -538]))[1] == 2                   # 1.5: the tie, to even (up)
    assert _bits(col([2.0 ** -537, 2.0 ** -537, 2.0 ** -538, 2.0 ** -538]))[1] == 2      # 2.5: the tie, to even (down)
    assert _bits(col([2.0 ** -537] * 3 + [2.0 ** -538]))[1] == 3
    assert _bits(col([2.0 ** -538]))[1] == 0 and _bits(col([2.0 ** -538, TINY]))[1] == 0
    got = col([1e200])
    assert got[0] == 1e200 and got[1] == INF and _bits(got)[2] == 0                      # s2 = +inf with s1 finite; one frame: d = 0
    got = col([1e200, 0.0])
    assert got[0] == 1e200 and got[1] == INF and got[2] == INF
    assert np.isnan(col([INF, 1.0, math.nan])).all() and np.isinf(col([INF, 1.0])).all() and np.isnan(col([1.0, math.nan])).all()
    assert (_bits(col([])) == 0).all() and (_bits(col([0.0, 0.0])) == 0).all()
    v = 0.1
    up = varianceref.one_ulp_up(v)
    got = col([v] * 999 + [up])
    ulp = Fraction(up) - Fraction(v)
    assert got[2] == float(999 * ulp * ulp) and got[2] > 0                               # W * S2 - S1^2 = (W - 1) * ulp^2 for one step
    for name, values in varianceref.columns():
        assert meanref.same(varianceref.dense_column(values), col(values)), name         # the integer form is the same reference
        assert meanref.same(col(values)[:1], [meanref.exact_sum(values)]), name          # out[0] is the mean's sum
    plane = np.array([[1.0, 5.0], [2.0, 5.0], [3.0, 5.0]])
    assert varianceref.expected(plane).tolist() == [[6.0, 15.0], [14.0, 75.0], [6.0, 0.0]]


def test_debug_variance_sums_is_the_reference_bit_for_bit(pkg):
    names = set()
    for name, values in varianceref.columns():
        names.add(name)
        want = varianceref.column(values)
        got = pkg.variance_sums(values)
        meanref.assert_same(got, want, name)
        if not np.isnan(want[0]):
            assert got[0] == pkg.binding.exact_sum(values), name                         # out[0] is the exact sum
            assert got[2] >= 0 and not np.signbit(got[2]), name
    assert {"full range", "denormals", "squares around the denormal grid", "tie in the denormal grid, up", "tie in the denormal grid, down",
            "DBL_MAX twice", "nan beats inf", "cell 0 shift 0", "cell 0 shift 15", "cell 0 shift 16", "cell 63 shift 16", "cell 31 shift 31",
            "cell 62 shift 1"} <= names
    assert list(pkg.variance_sums([1.0, 2.0, 3.0])) == [6.0, 14.0, 6.0]
    assert list(pkg.variance_sums([BIG, BIG])) == [INF, INF, 0.0] and list(pkg.variance_sums([1e200])) == [1e200, INF, 0.0]
    assert _bits(pkg.variance_sums([2.0 ** -537] * 2))[1] == 2


@pytest.mark.parametrize("length", [1, 2, 1000])
def test_a_constant_row_has_no_variance_at_all(pkg, length):
    for v in (0.1, 1.0 / 3.0, BIG, TINY, 2.0 ** -537, 1e-200, 1e150):
        got = pkg.variance_sums([v] * length)
        assert _bits(got)[2] == 0, (v, length)
        meanref.assert_same(got, varianceref.column([v] * length), "constant %r x %d" % (v, length))


def test_one_ulp_in_one_frame_is_seen_exactly_where_f64_sees_noise(pkg):
    seen = 0
    for v in (0.1, 1234.5678e-3, 1.0 / 3.0, 7e-10, 3e12):
        values = np.full(1000, v)
        values[137] = varianceref.one_ulp_up(v)
        want = varianceref.column(values)
        got = pkg.variance_sums(values)
        meanref.assert_same(got, want, "one ulp at %r" % v)
        assert got[2] > 0
        naive = values.size * np.sum(values * values) - np.sum(values) ** 2            # the one-pass f64 form: rounding noise
        assert naive != got[2], (v, naive, got[2])
        seen += 1
    assert seen == 5


def _expected_launch(n, frames, cu):
    """The rule restated: bands of 32 rows; about 6 workgroups per CU - two rounds of the three that fit its LDS - and no piece below 32
    frames; equal pieces, the last one shorter."""
    bands = (n + 31) // 32
    pieces = max(1, min((6 * cu + bands - 1) // bands, (frames + 31) // 32))
    return bands, pieces, (frames + pieces - 1) // pieces


@pytest.mark.parametrize("cu", [1, 64, 256, 304])
def test_debug_variance_launch_follows_the_rule(pkg, cu):
    b = pkg.binding
    for n in (1, 2, 31, 32, 33, 100, 256, 1024, 8192, 1 << 20):
        for frames in (1, 2, 31, 32, 33, 257, 2048, 16384, 1 << 24):
            got = b.debug_variance_launch(n, frames, cu)
            assert got == _expected_launch(n, frames, cu), (n, frames, cu)
            bands, pieces, per = got
            assert pieces * per >= frames and per >= 1                                   # every frame has a piece (a last piece may be empty)
            assert pieces <= 65535 and bands <= 1 << 15
    assert b.debug_variance_launch(1024, 16384, 256) == (32, 48, 342)
    assert b.debug_variance_launch(1024, 16384, 1) == (32, 1, 16384)


def _hex(values):
    return " ".join("%x" % b for b in np.ascontiguousarray(values, np.float64).view(np.uint64))


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/sp_variance_core.h over csrc/sp_exact_sum.h, host compiler, -fsanitize=address,undefined: the rows through stdin, the bits
    against varianceref.  The program adds every row in two orders and split across two accumulators merged cell by cell, and puts
    every value's five pieces back together against the 128-bit square."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "variance_core_check")
    csrc = os.path.join(ROOT, "spectroplot-js_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # (the runtimes linked in)
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "variance_core_check.cpp")])
    lines, want, names = [], [], []
    for name, values in varianceref.columns():
        lines.append("row %d %s" % (values.size, _hex(values)))
        want.append(varianceref.column(values))
        names.append(name)
    refused = ["row 2 %s" % _hex([1.0, -1.0]), "row 1 %s" % _hex([-0.0])]
    run = subprocess.run([exe], input="\n".join(lines + refused) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(lines) + len(refused) + 1 and got[-1] == ""
    for name, g, w in zip(names, got, want):
        bits = np.array([int(t, 16) for t in g.split()], np.uint64)
        meanref.assert_same(bits.view(np.float64), w, name)
    assert got[len(lines):-1] == ["refused"] * len(refused)
