"""The exact lagged covariance sums without a device: the ABI and its refusals, tests/lagcovref.py against hand-checked values,
sp_debug_lagcov - the host side of the code the kernels run - bit for bit against lagcovref, directly and through a stand-alone
program built with the address and undefined-behaviour sanitizers (tests/cpp/lagcov_core_check.cpp), the identities that tie it to the
variance sums, and the launch rule of the accumulation restated."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import lagcovref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_series_lagcov", "sp_power_lagcov", "sp_plan_execute_lagcov", "sp_render_lagcov", "sp_plan_lagcov_kernel_name_for",
                "sp_debug_lagcov", "sp_debug_lagcov_launch")
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
    for decl in ("#define SP_MAX_LAG_PAIRS 16", "#define SP_MAX_LAGS 1024",
                 "int sp_series_lagcov(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const int32_t *pairs, "
                 "int32_t npairs, int32_t lags, double *d_out);",
                 "int sp_power_lagcov(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, "
                 "const int32_t *pairs, int32_t npairs, int32_t lags, double *d_out);",
                 "int sp_plan_execute_lagcov(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, "
                 "int32_t count, const int32_t *pairs, int32_t npairs, int32_t lags, double *d_out);",
                 "int sp_render_lagcov(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, "
                 "const int32_t *bands, int32_t count, const int32_t *pairs, int32_t npairs, int32_t lags, double *out);",
                 "const char *sp_plan_lagcov_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);",
                 "int sp_debug_lagcov(const double *a, const double *b, int32_t width, int32_t lags, double *out);",
                 "int sp_debug_lagcov_launch(int32_t npairs, int32_t lags, int64_t terms, int32_t cu_count, int64_t *out, size_t capacity, "
                 "size_t *used);"):
        assert decl in flat, decl
    text = hdr[hdr.index("Exact lagged covariances of band-power series"):hdr.index("#define SP_MAX_LAG_PAIRS")]
    text = " ".join(text.replace("\n *", " ").split())
    for word in ("double[3][npairs][lags]", "N * P - A * B", "SIGNED", "never -0.0", "DENORMAL", "A NaN IS ANY NaN", "by presence",
                 "SP_ERR_UNSUPPORTED", "SP_ERR_INVALID_ARG", "NOR ON THE CU COUNT", "MEMORY", "Out of scope", "negative lags", "FFT-based"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_lagcov", "lagcov_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_lagcov", "power_lagcov", "series_lagcov"):
        assert hasattr(pkg.Context, name), name
    for name in ("lagcov_sums", "lagcov_terms", "lag_correlation"):
        assert callable(getattr(pkg, name)) and getattr(pkg.binding, name) is getattr(pkg, name) and name in pkg.__all__, name
    b = pkg.binding
    assert (b.SP_MAX_LAG_PAIRS, b.SP_MAX_LAGS) == (16, 1024)
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56      # no existing structure changed


def test_bad_arguments_are_refused_without_a_device(pkg):
    L = pkg.Library.get().L
    pairs = np.array([0, 0], np.int32)
    vp = C.c_void_p
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    out = np.full(12, 7.0)
    assert L.sp_series_lagcov(None, None, 1, 4, p(pairs), 1, 1, p(out)) == -1
    assert L.sp_power_lagcov(None, None, 4, 0, None, 0, None, 0, 1, None) == -1
    assert L.sp_plan_execute_lagcov(None, None, 0, 0, None, 0, None, 0, 1, None) == -1
    assert L.sp_render_lagcov(None, None, None, 0, 0, None, 0, None, 0, 1, None) == -1
    assert L.sp_plan_lagcov_kernel_name_for(None, 0, 0) == b""
    v = np.array([1.0, 2.0, 3.0])
    dl = L.sp_debug_lagcov
    assert dl(p(v), p(v), 3, 1, None) == -1
    assert dl(None, p(v), 3, 1, p(out)) == -1 and dl(p(v), None, 3, 1, p(out)) == -1
    assert dl(p(v), p(v), -1, 1, p(out)) == -1
    for lags in (0, -1, 1025):
        assert dl(p(v), p(v), 3, lags, p(out)) == -1
    for bad in (-1.0, -0.0, -INF, -TINY):
        w = np.array([1.0, bad, 2.0])
        assert dl(p(w), p(v), 3, 1, p(out)) == -1 and dl(p(v), p(w), 3, 1, p(out)) == -1
    assert (out == 7.0).all()                                           # a refusal writes nothing
    assert dl(p(v), p(v), 3, 2, p(out)) == 0                            # N = 2: lag 0 is (1, 2)(1, 2), lag 1 is (1, 2)(2, 3)
    assert list(out[:8]) == [5.0, 8.0, 1.0, 1.0, 3.0, 5.0, 7.0, 7.0]    # 2 * 5 - 3 * 3, 2 * 8 - 3 * 5; six values and no more
    assert dl(None, None, 0, 3, p(out)) == 0 and (_bits(out[:9]) == 0).all() and (out[9:] == 7.0).all()   # no frames: 3 * lags times +0.0
    assert np.isnan(pkg.lagcov_sums([1.0, -math.nan], [1.0, 2.0], 1)).all()     # a negative NaN is a NaN
    with pytest.raises(pkg.SpectroplotError):
        pkg.lagcov_sums([1.0, 2.0], [1.0], 1)
    used = C.c_size_t()
    grid = np.zeros(3, np.int64)
    for npairs, lags, terms, cu in ((0, 1, 1, 1), (17, 1, 1, 1), (1, 0, 1, 1), (1, 1025, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert L.sp_debug_lagcov_launch(npairs, lags, terms, cu, p(grid), 3, C.byref(used)) == -1
    assert L.sp_debug_lagcov_launch(1, 64, 64, 8, p(grid), 2, C.byref(used)) == -1 and used.value == 3
    assert L.sp_debug_lagcov_launch(1, 64, 64, 8, p(grid), 3, None) == -1 and not grid.any()
    assert [pkg.lagcov_terms(w, l) for w, l in ((0, 1), (1, 1), (5, 2), (5, 5), (5, 6), (16384, 1024))] == [0, 1, 4, 1, 0, 15361]


def test_reference_against_hand_checked_values():
    pair = lagcovref.pair
    # two frames: lag 0 of (1, 2) with (3, 5): P = 13, 2 * 13 - 3 * 8 = 2, B = 8
    assert pair([1.0, 2.0], [3.0, 5.0], 1).ravel().tolist() == [13.0, 2.0, 8.0]
    # ... and at lags = 2 one term per lag, whose covariance is zero
    got = pair([1.0, 2.0], [3.0, 5.0], 2)
    assert got.tolist() == [[3.0, 5.0], [0.0, 0.0], [3.0, 5.0]] and (_bits(got[1]) == 0).all()
    # a negative covariance: a rises where b falls, 3 * 10 - 6 * 6 = -6
    got = pair([1.0, 2.0, 3.0], [3.0, 2.0, 1.0], 1)
    assert got.ravel().tolist() == [10.0, -6.0, 6.0] and np.signbit(got[1, 0])
    # a constant series: +0.0 with a clear sign bit, whatever the other series does
    for c in (0.1, 1.0 / 3.0, BIG, TINY):
        got = pair([c] * 7, [c] * 7, 3)
        assert (_bits(got[1]) == 0).all(), c
        got = pair([c] * 7, np.arange(7.0), 3)
        assert (_bits(got[1]) == 0).all(), c
    # a denormal result: P = 2^-1074 exactly and N * P - A * B = 2 * 2^-1074 - 2^-1074 = 2^-1074; and one below the grid, tied to even
    got = pair([2.0 ** -537, 0.0], [2.0 ** -537, 0.0], 1)
    assert _bits(got).ravel().tolist() == [1, 1, int(_bits([2.0 ** -537])[0])]
    assert _bits(pair([2.0 ** -538, 0.0], [2.0 ** -537, 0.0], 1))[0, 0] == 0            # half a denormal: the tie, to even (down)
    assert _bits(pair([2.0 ** -538 * 3, 0.0], [2.0 ** -537, 0.0], 1))[0, 0] == 2        # 1.5: the tie, to even (up)
    got = pair([0.0, 2.0 ** -537], [2.0 ** -537, 0.0], 1)
    assert got[0, 0] == 0.0 and _bits(got)[1, 0] == (1 << 63) | 1                       # -2^-1074: a negative denormal
    # ... and a negative value below half a denormal keeps its sign as it rounds to zero: only an EXACT zero is +0.0
    assert _bits(pair([0.0, 2.0 ** -538], [2.0 ** -538, 0.0], 1))[1, 0] == 1 << 63
    # past DBL_MAX of either sign
    got = pair([BIG, 0.0], [BIG, 0.0], 1)
    assert got.ravel().tolist() == [INF, INF, BIG]
    got = pair([BIG, 0.0], [0.0, BIG], 1)
    assert got.ravel().tolist() == [0.0, -INF, BIG]
    # the special values by window membership: N = 3, a NaN at b[3] marks the lags >= 1, an inf at a[3] lies outside a's window
    a, b = np.array([1.0, 2.0, 3.0, INF]), np.array([1.0, 1.0, 1.0, math.nan])
    got = pair(a, b, 2)
    assert np.isfinite(got[:, 0]).all() and np.isnan(got[:, 1]).all()
    got = pair([0.0, 0.0, 5.0], [INF, 1.0, 1.0], 1)
    assert np.isinf(got).all() and (got > 0).all()                                       # 0 * inf is marked +inf: presence, not arithmetic
    assert np.isnan(pair([INF, 1.0], [math.nan, 1.0], 1)).all()                          # NaN beats inf
    assert (_bits(pair([1.0, 2.0], [3.0, 4.0], 3)) == 0).all()                           # lags > width: N = 0
    assert (_bits(pair([], [], 1)) == 0).all()
    # float() of a Fraction rounds correctly into the denormal range
    assert float(Fraction(5e-324) * Fraction(3, 2)) == 1e-323
    # expected() lays the pairs out [3, npairs, lags]
    s = np.array([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]])
    got = lagcovref.expected(s, [(0, 1), (1, 0), (0, 0)], 1)
    assert got.shape == (3, 3, 1) and got[:, :, 0].tolist() == [[10.0, 10.0, 14.0], [-6.0, -6.0, 6.0], [6.0, 6.0, 6.0]]


def _cases():
    """(name, a, b, lags) of the series sp_debug_lagcov and the stand-alone program see."""
    rng = np.random.default_rng(2026)
    full = 0x000fffffffffffff
    f = lagcovref._f
    cases = [("two frames", [1.0, 2.0], [3.0, 5.0], 1), ("negative", [1.0, 2.0, 3.0], [3.0, 2.0, 1.0], 1),
             ("lags > width", [1.0, 2.0], [3.0, 4.0], 3), ("lags == width", [1.0, 2.0, 4.0], [3.0, 4.0, 9.0], 3), ("empty", [], [], 2),
             ("one frame", [3.5], [2.5], 1), ("zeros", [0.0] * 9, [0.0] * 9, 4),
             ("a zero operand", [0.0, 3.0, 0.0, 1.0, 7.0, 0.0], [2.0, 0.0, 0.0, 5.0, 0.0, 4.0], 3),
             ("only A * B", [1.0, 0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 1.0, 0.0], 2),
             ("DBL_MAX", [BIG, BIG, 1.0], [BIG, TINY, BIG], 2), ("DBL_MAX against zero", [BIG, 0.0], [0.0, BIG], 1),
             ("DBL_MAX and denormals", [BIG, TINY, BIG, 1.0, TINY], [TINY, BIG, 1.0, BIG, BIG], 2),
             ("denormal result", [2.0 ** -537, 0.0], [2.0 ** -537, 0.0], 1), ("negative denormal", [0.0, 2.0 ** -537], [2.0 ** -537, 0.0], 1),
             ("tie below the grid", [2.0 ** -538, 0.0], [2.0 ** -537, 0.0], 1), ("tie, up", [2.0 ** -538 * 3, 0.0], [2.0 ** -537, 0.0], 1),
             ("constant", [0.1] * 40, [0.1] * 40, 9), ("constant against a ramp", [1.0 / 3.0] * 40, np.arange(40.0), 9),
             ("pedestal", lagcovref.pedestal_series(), lagcovref.pedestal_series(), 17)]
    for k in range(4):
        w = (5, 40, 70, 130)[k]
        cases.append(("full range %d" % k, lagcovref.full_range(rng, w), lagcovref.full_range(rng, w), (1, 7, 33, 40)[k]))
        cases.append(("clustered %d" % k, lagcovref.clustered(rng, w, 10.0 ** (40 * k - 60)), lagcovref.clustered(rng, w, 3.0), (2, 8, 32, 65)[k]))
    cases.append(("denormals", lagcovref.from_fields(rng, np.zeros(50, np.int64), 50), lagcovref.from_fields(rng, np.zeros(50, np.int64), 50), 5))
    # exponent sums that hit every shift 0 .. 31, both parities: a's e - 1 fixed, b's e - 1 runs over 64 neighbours, lag 0 .. 2
    for ea in (1, 700, 1023, 2046):
        eb0 = 1 if ea > 1 else 900
        eb = np.minimum(eb0 + np.arange(70), 2046)
        a = np.array([f((ea << 52) | full), f(ea << 52), f((ea << 52) | 1)] * 24, np.float64)[:70]
        b = ((eb.astype(np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, 70, dtype=np.uint64)).view(np.float64)
        cases.append(("shifts from e = %d" % ea, a, b, 3))
    # a NaN or an inf at each window edge: N = 6, lags = 5, width = 10
    base_a, base_b = 1.0 + rng.random(10), 1.0 + rng.random(10)
    for name, special in (("nan", math.nan), ("inf", INF)):
        for at in (0, 5, 6, 9):
            a, b = base_a.copy(), base_b.copy()
            a[at] = special
            cases.append(("%s at a[%d]" % (name, at), a, base_b, 5))
            b[at] = special
            cases.append(("%s at b[%d]" % (name, at), base_a, b, 5))
    a, b = base_a.copy(), base_b.copy()
    a[2], b[7] = INF, math.nan
    cases.append(("inf in a, nan in b", a, b, 5))
    return [(name, np.array(a, np.float64), np.array(b, np.float64), lags) for name, a, b, lags in cases]


def test_debug_lagcov_is_the_reference_bit_for_bit(pkg):
    shifts = set()
    for name, a, b, lags in _cases():
        want = lagcovref.pair(a, b, lags)
        lagcovref.assert_same(pkg.lagcov_sums(a, b, lags), want, name)
        lagcovref.assert_same(pkg.lagcov_sums(b, a, lags), lagcovref.pair(b, a, lags), name + ", swapped")
        if name.startswith("shifts"):
            ea = (_bits(a) >> np.uint64(52)).astype(np.int64) - 1
            eb = (_bits(b) >> np.uint64(52)).astype(np.int64) - 1
            n = a.size - lags + 1
            for l in range(lags):
                shifts |= {int(e) & 31 for e in ea[:n] + eb[l:l + n]}
    assert shifts == set(range(32))                                                      # every shift of a product, odd ones included
    # the window edges mark exactly the lags they should: N = 6, lags = 5
    cases = {name: (a, b) for name, a, b, _ in _cases()}
    nan_lags = lambda name: np.isnan(pkg.lagcov_sums(*cases[name], 5)).all(axis=0).tolist()  # noqa: E731
    inf_lags = lambda name: np.isinf(pkg.lagcov_sums(*cases[name], 5)).all(axis=0).tolist()  # noqa: E731
    assert nan_lags("nan at a[0]") == [True] * 5 and nan_lags("nan at a[5]") == [True] * 5
    assert nan_lags("nan at a[6]") == [False] * 5 and nan_lags("nan at a[9]") == [False] * 5
    assert nan_lags("nan at b[0]") == [True, False, False, False, False]
    assert nan_lags("nan at b[5]") == [True] * 5                                         # b[N + l0 - 1] with l0 = 0
    assert nan_lags("nan at b[6]") == [False, True, True, True, True]                    # ... with l0 = 1
    assert nan_lags("nan at b[9]") == [False, False, False, False, True]
    assert inf_lags("inf at b[6]") == [False, True, True, True, True] and inf_lags("inf at a[6]") == [False] * 5
    got = pkg.lagcov_sums(*cases["inf in a, nan in b"], 5)
    assert np.isinf(got[:, :2]).all() and np.isnan(got[:, 2:]).all()                     # b[7] is in the window from lag 2 on
    # the hand-checked values again, through the library
    assert pkg.lagcov_sums([1.0, 2.0, 3.0], [3.0, 2.0, 1.0], 1).ravel().tolist() == [10.0, -6.0, 6.0]
    assert pkg.lagcov_sums([BIG, 0.0], [0.0, BIG], 1).ravel().tolist() == [0.0, -INF, BIG]
    assert _bits(pkg.lagcov_sums([0.0, 2.0 ** -537], [2.0 ** -537, 0.0], 1))[1, 0] == (1 << 63) | 1
    assert (_bits(pkg.lagcov_sums([0.1] * 40, np.arange(40.0), 9)[1]) == 0).all()        # +0.0, never -0.0


def test_identity_with_the_variance_sums(pkg):
    """Pair (a, a) at lags = 1 is the variance: out[0] = S2, out[1] = W * S2 - S1^2, out[2] = S1."""
    import varianceref
    seen = 0
    for name, values in varianceref.columns():
        if values.size == 0:
            continue
        got, var = pkg.lagcov_sums(values, values, 1)[:, 0], pkg.variance_sums(values)
        lagcovref.assert_same(got, np.array([var[1], var[2], var[0]]), name)
        seen += 1
    assert seen > 40


def test_lag_zero_is_symmetric(pkg):
    """Lag 0 of (a, b) and of (b, a): the same P and the same N * P - A * B, bit for bit."""
    for name, a, b, lags in _cases():
        if a.size == 0 or np.isnan(a).any() or np.isnan(b).any() or np.isinf(a).any() or np.isinf(b).any():
            continue
        ab, ba = pkg.lagcov_sums(a, b, 1), pkg.lagcov_sums(b, a, 1)
        assert np.array_equal(_bits(ab[:2]), _bits(ba[:2])), name


def test_the_pedestal_is_seen_exactly_where_f64_sees_noise(pkg):
    """257 frames of 1e6 + 1e-6 * square(period 8) + 1e-9 * noise: the exact autocovariance is a clean period-8 wave, the one-pass f64
    form is rounding noise fifteen orders of magnitude above it."""
    a = lagcovref.pedestal_series(257)
    lags = 17
    n = pkg.lagcov_terms(a.size, lags)
    got = pkg.lagcov_sums(a, a, lags)
    lagcovref.assert_same(got, lagcovref.pair(a, a, lags), "pedestal")
    cov = got[1] / np.float64(n * n)
    assert (cov[[0, 8, 16]] > 2.4e-13).all() and (cov[[4, 12]] < -2.4e-13).all() and (np.abs(cov) < 2.6e-13).all()
    assert (np.abs(cov[[2, 6, 10, 14]]) < 1e-14).all()                                   # the zero crossings of a period of 8
    for l in range(lags):
        naive = n * np.dot(a[:n], a[l:l + n]) - a[:n].sum() * a[l:l + n].sum()
        assert naive != got[1, l], (l, naive, got[1, l])
    r = pkg.lag_correlation(got[1], got[1, 0], got[1, 0])
    assert r[0] == 1.0 and abs(r[4] + 1.0) < 1e-4 and abs(r[8] - 1.0) < 1e-4


def _expected_launch(npairs, lags, terms, cu):
    """The rule restated: a band is a pair and 32 lags; about 6 workgroups per CU - two rounds of the three that fit its LDS - and no
    piece below 32 terms; equal pieces, the last one shorter."""
    bands = npairs * ((lags + 31) // 32)
    pieces = max(1, min((6 * cu + bands - 1) // bands, (terms + 31) // 32))
    return bands, pieces, (terms + pieces - 1) // pieces


@pytest.mark.parametrize("cu", [1, 64, 256, 304])
def test_debug_lagcov_launch_follows_the_rule(pkg, cu):
    b = pkg.binding
    for npairs in (1, 3, 16):
        for lags in (1, 2, 31, 32, 33, 65, 1024):
            for terms in (1, 2, 31, 32, 33, 257, 1031, 15361, (1 << 31) - 1):
                got = b.debug_lagcov_launch(npairs, lags, terms, cu)
                assert got == _expected_launch(npairs, lags, terms, cu), (npairs, lags, terms, cu)
                bands, pieces, per = got
                assert pieces * per >= terms and per >= 1                                # every term has a piece (a last piece may be empty)
                assert pieces <= 65535 and bands <= 512
    assert b.debug_lagcov_launch(1, 64, 16321, 256) == (2, 511, 32)
    assert b.debug_lagcov_launch(16, 1024, 15361, 256) == (512, 3, 5121)
    assert b.debug_lagcov_launch(16, 1024, 15361, 1) == (512, 1, 15361)


def _hex(values):
    return " ".join("%x" % b for b in np.ascontiguousarray(values, np.float64).view(np.uint64))


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/sp_lagcov_core.h over csrc/sp_variance_core.h and csrc/sp_exact_sum.h, host compiler, -fsanitize=address,undefined: the
    series through stdin, the bits against lagcovref.  The program accumulates every lag in two orders and split across two
    accumulators merged cell by cell, and puts every term's five pieces back together against the 128-bit product and its shift; the
    cases hold negative and zero differences."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lagcov_core_check")
    csrc = os.path.join(ROOT, "spectroplot-js_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # (the runtimes linked in)
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "lagcov_core_check.cpp")])
    lines, want, names = [], [], []
    negative = zero = 0
    for name, a, b, lags in _cases():
        lines.append(("pair %d %d %s %s" % (a.size, lags, _hex(a), _hex(b))).strip())
        w = lagcovref.pair(a, b, lags)
        negative += int(np.signbit(w[1]).sum())
        zero += int((_bits(w[1]) == 0).sum())
        want.append(w)
        names.append(name)
    assert negative > 20 and zero > 20
    refused = ["pair 2 1 %s %s" % (_hex([1.0, -1.0]), _hex([1.0, 1.0])), "pair 1 1 %s %s" % (_hex([0.0]), _hex([-0.0])),
               "pair 1 0 %s %s" % (_hex([1.0]), _hex([1.0])), "pair 1 1025 %s %s" % (_hex([1.0]), _hex([1.0]))]
    run = subprocess.run([exe], input="\n".join(lines + refused) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")
    assert len(got) == len(lines) + len(refused) + 1 and got[-1] == ""
    for name, g, w in zip(names, got, want):
        bits = np.array([int(t, 16) for t in g.split()], np.uint64)
        lagcovref.assert_same(bits.view(np.float64).reshape(w.shape), w, name)
    assert got[len(lines):-1] == ["refused"] * len(refused)
