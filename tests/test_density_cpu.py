"""The persistence spectrum (sp_*_density) without a device: the ABI, the counting kernel's decomposition, and tests/densityref.py
against the oracle's own histogram."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityref
import siggen
import test_launch_shapes_gpu as base
from __graft_entry__ import ROOT, build, load_package
from oracle import pyoracle

ENTRY_POINTS = ("sp_density_from_index", "sp_plan_execute_density", "sp_render_density", "sp_debug_density_launch")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def test_header_declares_and_library_exports_and_binds_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
    sec = hdr[hdr.index("Persistence spectrum"):hdr.index("int sp_density_from_index(")]
    assert "SP_ERR_UNSUPPORTED" in sec and "SP_ERR_INVALID_ARG" in sec
    assert "width * n bytes" in sec and "grown and never shrunk" in sec          # the workspace cost
    assert "wraps modulo 2^32" in sec                                            # accumulate
    assert sec.count("worker.js:105-117") >= 4                                   # every declaration cites the reference
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for cls, names in ((pkg.Plan, ("execute_density",)), (pkg.Context, ("render_density", "density_from_index")),
                       (pkg.Library, ("debug_density_launch",))):
        for name in names:
            assert hasattr(cls, name), name
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56     # no structure changed


def test_entry_points_without_a_context_or_plan(pkg):
    """No object to work on: the statuses sp_plan_execute_index gives (SP_ERR_NO_DEVICE without a device, SP_ERR_INVALID_ARG with one)."""
    L = pkg.Library.get().L
    want = -5 if pkg.Library.get().device_count() == 0 else -1
    assert L.sp_plan_execute_index(None, None, 0, 0, None, None) == want
    assert L.sp_plan_execute_density(None, None, 0, 0, None, 0) == want
    assert L.sp_render_density(None, None, None, 0, 0, None) == want
    assert L.sp_density_from_index(None, None, 1, 0, 0, 1, None, 0) == want


def _shapes(count, seed):
    rng = np.random.default_rng(seed)
    out = [(1, 1, 0, 1), (1, 0, 0, 0), (2, 5, 0, 5), (64, 2048, 0, 2048), (64, 2049, 0, 2049), (65, 1025, 1, 1025), (8, 4097, 0, 4097)]
    while len(out) < count:
        n = int(rng.choice([1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 100, 128, 200, 256]))
        width = int(rng.choice([int(rng.integers(0, 40)), int(rng.integers(0, 9000)), 1024, 2048, 2049, 4096]))
        a, b = sorted(int(v) for v in rng.integers(0, width + 1, 2))
        out.append((n, width, a, b) if rng.integers(0, 3) else (n, width, 0, width))
    return out


@pytest.mark.parametrize("waterfall", [False, True])
def test_the_decomposition_covers_the_range_exactly_once(pkg, waterfall):
    """Over a few hundred shapes: the workgroups' rectangles tile [0, n) x [x_begin, x_end) - every pixel in exactly one - none is empty,
    none exceeds rows x frames, and the six header words agree with them.  The grid does not depend on where the image sits: the entry
    takes no pointer."""
    lib = pkg.Library.get()
    for n, width, a, b in _shapes(300, 7 + waterfall):
        d = lib.debug_density_launch(n, width, waterfall, a, b)
        what = (n, width, a, b, waterfall)
        assert d["workgroups"] == len(d["rects"]) == d["bands"] * d["pieces"], what
        assert d["bands"] == -(-n // d["rows"]) and d["pieces"] == -(-(b - a) // d["frames"]), what
        assert d["lds_bytes"] == 1024 * d["rows"] <= 64 << 10, what           # u32[256] per row, inside a workgroup's 64 KiB
        seen = np.zeros((n, b - a), np.int32)
        for y0, y1, x0, x1 in d["rects"].tolist():
            assert 0 <= y0 < y1 <= n and a <= x0 < x1 <= b and y1 - y0 <= d["rows"] and x1 - x0 <= d["frames"], (what, (y0, y1, x0, x1))
            seen[y0:y1, x0 - a:x1 - a] += 1
        assert (seen == 1).all(), what


def test_debug_launch_refuses_a_short_buffer_and_says_what_it_needs(pkg):
    L = pkg.Library.get().L
    used = C.c_size_t(0)
    out = np.full(64, -7, np.int64)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.sp_debug_density_launch(64, 5000, 0, 0, 5000, p, 5, C.byref(used)) == -1
    assert used.value == 6 + 4 * 8 * 3 and (out == -7).all()                    # 8 bands of 8 rows x 3 pieces of 2048 frames
    assert L.sp_debug_density_launch(64, 2500, 1, 0, 2500, p, 6 + 4 * 5 - 1, C.byref(used)) == -1
    assert used.value == 6 + 4 * 1 * 5 and (out == -7).all()                    # 1 band of 64 rows x 5 pieces of 512 frames
    assert L.sp_debug_density_launch(64, 2500, 1, 0, 2500, p, 6 + 4 * 5, C.byref(used)) == 0 and out[0] == 5
    for bad in ((0, 5, 0, 5), (4, -1, 0, 0), (4, 5, -1, 5), (4, 5, 3, 2), (4, 5, 0, 6)):
        assert L.sp_debug_density_launch(bad[0], bad[1], 0, bad[2], bad[3], p, 64, C.byref(used)) == -1, bad


@pytest.mark.parametrize("waterfall", [False, True])
def test_densityref_reproduces_c_hist_and_row_sums_on_an_oracle_reply(waterfall):
    n, fmt, W, lut = 64, "CS16", 37, base._lut()
    data = siggen.generate(fmt, base.GEN, n + 36 * 50 + 3)
    win, weight = pyoracle.window("hann", n)
    want = pyoracle.render(fmt, data, n, win, 1.0 / weight, base.GAIN, base.RANGE, lut, W, False, waterfall)
    d = densityref.expected(want, n, len(lut), W, waterfall)
    assert d.dtype == np.uint32 and d.shape == (n, 256)
    assert (d.sum(axis=1) == W).all()
    assert np.array_equal(d.sum(axis=0), want["c_hist"])
    assert np.array_equal(d, densityref.count_image(want["rgba"].reshape(-1, 4)[:, 0], n, W, waterfall, 256))
    # the two layouts of one request draw the same rows: the array is the same
    other = pyoracle.render(fmt, data, n, win, 1.0 / weight, base.GAIN, base.RANGE, lut, W, False, not waterfall)
    assert np.array_equal(d, densityref.expected(other, n, len(lut), W, not waterfall))
    # count_image drops the bytes the map does not have
    cut = densityref.count_image(want["rgba"].reshape(-1, 4)[:, 0], n, W, waterfall, 100)
    assert cut.shape == (n, 100) and np.array_equal(cut, d[:, :100])
