"""The exact mean-power trace without a device: the exact-sum core (csrc/sp_exact_sum.h) against math.fsum, bit for bit - through the
library's host side (sp_debug_exact_sum) and through a stand-alone program built with the address and undefined-behaviour sanitizers
(tests/cpp/exact_sum_check.cpp) - and the ABI."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import meanref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_power_mean", "sp_plan_execute_mean", "sp_render_mean", "sp_context_set_mean_window", "sp_debug_exact_sum",
                "sp_plan_mean_kernel_name_for")
DBL_MAX = sys.float_info.max
TINY = 5e-324


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def _pattern(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _same(got, want):
    return (got != got and want != want) or _pattern(got) == _pattern(want)


def _field(e, frac=0x000fffffffffffff):
    return struct.unpack("<d", struct.pack("<Q", (e << 52) | frac))[0]


def hand_made():
    """The lists the feature's issue names, each with a word for the failure message."""
    lists = [("empty", []), ("zeros", [0.0, 0.0]),
             ("tie to even", [2.0 ** 53, 1.0]), ("sticky bit", [2.0 ** 53, 1.0, TINY]), ("above the tie", [2.0 ** 53, 3.0]),
             ("seven denormals", [TINY] * 7), ("denormal boundary", [2.0 ** -1022, TINY]),
             ("overflow", [DBL_MAX, DBL_MAX]), ("just below overflow", [DBL_MAX, 2.0 ** 969]),
             ("rounds to overflow", [DBL_MAX, 2.0 ** 970]),
             ("carries", [math.nextafter(2.0, 1.0)] * (1 << 20))]
    for cell in (0, 1, 62, 63):
        for s in (0, 1, 30, 31):
            e = 32 * cell + s + 1
            if e > 2046:
                continue
            lists.append(("cell %d shift %d" % (cell, s), [_field(e)]))
            lists.append(("cell %d shift %d, thrice and a tiny one" % (cell, s), [_field(e)] * 3 + [TINY]))
            lists.append(("cell %d shift %d and its neighbours" % (cell, s), [_field(e), _field(max(e - 1, 0)), _field(min(e + 1, 2046), 1)]))
    lists.append(("every boundary", meanref.boundary_values()))
    return lists


def random_lists(seed=20261019, count=3000):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        out.append(("random %d" % k, list(meanref.random_values(rng, int(rng.integers(1, 41))))))
        out.append(("clustered %d" % k, list(meanref.random_values(rng, int(rng.integers(1, 41)), clustered=True))))
    return out


SPECIALS = [("one NaN", [1.0, math.nan, 2.0], math.nan), ("NaN beats inf", [math.inf, math.nan], math.nan),
            ("NaN beats overflow", [DBL_MAX, DBL_MAX, math.nan], math.nan), ("one inf", [1.0, math.inf, 2.0], math.inf),
            ("two infs", [math.inf, math.inf], math.inf), ("inf alone", [math.inf], math.inf)]


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    for decl in ("int sp_power_mean(sp_context *ctx, const double *d_power, int32_t n, int32_t width, double *d_mean);",
                 "int sp_plan_execute_mean(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_mean);",
                 "int sp_render_mean(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db, "
                 "double *mean);",
                 "int sp_context_set_mean_window(sp_context *ctx, size_t bytes);",
                 "int sp_debug_exact_sum(const double *values, size_t count, double *sum);",
                 "const char *sp_plan_mean_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);"):
        assert decl in hdr, decl
    text = hdr[hdr.index("Exact mean-power trace"):hdr.index("int sp_power_mean(")]
    for word in ("SP_ERR_UNSUPPORTED", "NaN", "math.fsum", "2^1024 - 2^970", "DOES NOT DEPEND ON THE CU COUNT", "544 MiB", "Out of scope"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_mean", "mean_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_mean", "power_mean", "set_mean_window"):
        assert hasattr(pkg.Context, name), name
    assert callable(pkg.binding.exact_sum)
    # no existing structure changed
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.DETECTORS == {"sample": 0, "peak": 1}


def test_null_handles_are_invalid_arguments(pkg):
    L = pkg.Library.get().L
    assert L.sp_power_mean(None, None, 4, 0, None) == -1
    assert L.sp_plan_execute_mean(None, None, 0, 0, None) == -1
    assert L.sp_render_mean(None, None, None, 0, 0, 0, None) == -1
    assert L.sp_context_set_mean_window(None, 0) == -1
    assert L.sp_plan_mean_kernel_name_for(None, 0, 0) == b""
    out = C.c_double()
    assert L.sp_debug_exact_sum(None, 0, None) == -1
    assert L.sp_debug_exact_sum(None, 3, C.byref(out)) == -1


def test_library_sums_the_hand_made_lists_as_fsum_does(pkg):
    for what, values in hand_made():
        got, want = pkg.binding.exact_sum(values), meanref.exact_sum(values)
        assert _same(got, want), (what, got, want)
    assert _pattern(pkg.binding.exact_sum([])) == 0                      # +0.0
    assert pkg.binding.exact_sum([DBL_MAX, DBL_MAX]) == math.inf
    assert pkg.binding.exact_sum([2.0 ** 53, 1.0]) == 2.0 ** 53 and pkg.binding.exact_sum([2.0 ** 53, 1.0, TINY]) == 2.0 ** 53 + 2
    assert pkg.binding.exact_sum([TINY] * 7) == 7 * TINY


def test_library_sums_random_lists_as_fsum_does(pkg):
    bad = [(what, values) for what, values in random_lists()
           if not _same(pkg.binding.exact_sum(values), meanref.exact_sum(values))]
    assert not bad, (len(bad), bad[0])


def test_library_sum_does_not_depend_on_the_order(pkg):
    rng = np.random.default_rng(7)
    for _ in range(50):
        v = meanref.random_values(rng, 40)
        first = _pattern(pkg.binding.exact_sum(v))
        assert first == _pattern(pkg.binding.exact_sum(v[::-1])) == _pattern(pkg.binding.exact_sum(np.sort(v)))


def test_nan_rule_inf_rule_and_negative_values(pkg):
    for what, values, want in SPECIALS:
        assert _same(pkg.binding.exact_sum(values), want), what
        assert _same(meanref.exact_sum(values), want), what
    for values in ([-1.0], [1.0, -TINY], [-0.0], [2.0, -math.inf]):
        with pytest.raises(pkg.SpectroplotError) as ei:
            pkg.binding.exact_sum(values)
        assert ei.value.status == -1, values


def test_reference_mean_of_a_plane():
    plane = np.array([[1.0, 2.0 ** 53, math.nan, math.inf, DBL_MAX, 0.0],
                      [2.0, 1.0, 1.0, 1.0, DBL_MAX, 0.0],
                      [4.0, TINY, 1.0, math.inf, 0.0, 0.0]])
    want = np.array([7.0 / 3, (2.0 ** 53 + 2) / 3, math.nan, math.inf, math.inf, 0.0])
    assert meanref.same(meanref.expected(plane), want)
    assert np.isnan(meanref.expected(np.zeros((0, 5)))).all() and meanref.expected(np.zeros((0, 5))).shape == (5,)
    assert not meanref.same(want, np.nextafter(want, 0.0)) and not meanref.same(want, want[:-1])
    # the synthetic planes of the GPU test hold what they are meant to hold
    p = meanref.synthetic_plane(1, 257, 64)
    assert (p >= 0).all() and np.isfinite(p).all() and (p[:, 2] < 2.0 ** -1022).all() and np.isinf(meanref.expected(p)[5])


def test_stand_alone_program_under_the_sanitizers_sums_as_fsum_does(tmp_path):
    """csrc/sp_exact_sum.h alone, host compiler, -fsanitize=address,undefined: every list of this file through stdin."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "exact_sum_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes linked in: nothing has to come first at load time)
                           "-I", os.path.join(ROOT, "spectroplot-js_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "exact_sum_check.cpp")])
    cases = [(w, v, meanref.exact_sum(v)) for w, v in hand_made() + random_lists(count=1000)] + SPECIALS
    cases += [("negative", [1.0, -1.0], None), ("minus zero", [-0.0], None)]
    text = "".join(" ".join("%x" % _pattern(float(x)) for x in v) + "\n" for _, v, _ in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split("\n")
    assert len(lines) == len(cases) + 1 and lines[-1] == ""
    for (what, values, want), line in zip(cases, lines):
        if want is None:
            assert line == "invalid", what
        else:
            got = struct.unpack("<d", struct.pack("<Q", int(line, 16)))[0]
            assert _same(got, want), (what, got, want)
