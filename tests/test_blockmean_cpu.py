"""The averaged spectrogram without a device: the ABI, the column arithmetic, the host side of the block means against math.fsum, the
split of a run of frames (csrc/sp_blockmean_core.h) on a grid and through a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/cpp/blockmean_core_check.cpp), and the colour index of sp_plan_power_to_index against the
reference's arithmetic at every edge."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import blockmeanref
import edgeref
import meanref
from __graft_entry__ import ROOT, build, load_package

ENTRY_POINTS = ("sp_blockmean_columns", "sp_power_blockmean", "sp_plan_execute_blockmean", "sp_render_blockmean",
                "sp_plan_blockmean_kernel_name_for", "sp_context_set_blockmean_direct_max", "sp_debug_blockmean",
                "sp_debug_blockmean_split", "sp_debug_blockmean_launch", "sp_plan_power_to_index", "sp_debug_gray_index")
DECLARATIONS = (
    "int32_t sp_blockmean_columns(int32_t width, int32_t group);",
    "int sp_power_blockmean(sp_context *ctx, const double *d_power, int32_t n, int32_t width, int32_t group, double *d_out);",
    "int sp_plan_execute_blockmean(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, int32_t group, double *d_out);",
    "int sp_render_blockmean(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t group,\n"
    "                        int32_t db, double *out);",
    "const char *sp_plan_blockmean_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);",
    "int sp_context_set_blockmean_direct_max(sp_context *ctx, int32_t frames);",
    "int sp_debug_blockmean(const double *values, int32_t n, int32_t width, int32_t group, double *out);",
    "int sp_debug_blockmean_split(int64_t x_base, int64_t frames, int32_t width, int32_t group, int32_t direct_max, int64_t *out, "
    "size_t capacity,\n                             size_t *used);",
    "int sp_plan_power_to_index(sp_plan *plan, const double *d_power, int32_t width, uint8_t *d_index);",
    "#define SP_BLOCKMEAN_DIRECT_FRAMES ",
)
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    for decl in DECLARATIONS:
        assert decl in hdr, decl
    text = hdr[hdr.index("Averaged spectrogram:"):hdr.index("int32_t sp_blockmean_columns(")]
    for word in ("ceil(width / group)", "count_c", "0x7ff8000000000000", "2^1024 - 2^970", "+0.0", "SP_ERR_UNSUPPORTED", "math.fsum",
                 "DOES NOT DEPEND ON THE CU COUNT", "group == 1", "group >= width", "SP_ERR_NOMEM", "NOT the mean of the\n *   dB values",
                 "Out of scope"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_blockmean", "blockmean_kernel_name_for", "power_to_index"):
        assert hasattr(pkg.Plan, name), name
    for name in ("render_blockmean", "power_blockmean", "set_blockmean_direct_max"):
        assert hasattr(pkg.Context, name), name
    for name in ("blockmean_columns", "blockmean", "blockmean_split", "gray_index"):
        assert callable(getattr(pkg.binding, name)), name
    for name in ("blockmean", "power_to_index"):
        assert name in open(os.path.join(ROOT, "spectroplot-js_amd", "tensor.py")).read()
    # no existing structure changed
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.DETECTORS == {"sample": 0, "peak": 1}


def test_null_handles_are_invalid_arguments(pkg):
    L = pkg.Library.get().L
    assert L.sp_power_blockmean(None, None, 4, 0, 1, None) == -1
    assert L.sp_plan_execute_blockmean(None, None, 0, 0, 1, None) == -1
    assert L.sp_render_blockmean(None, None, None, 0, 0, 1, 0, None) == -1
    assert L.sp_context_set_blockmean_direct_max(None, 0) == -1
    assert L.sp_plan_power_to_index(None, None, 0, None) == -1
    assert L.sp_plan_blockmean_kernel_name_for(None, 0, 0) == b""
    used = C.c_size_t()
    assert L.sp_debug_blockmean(None, 4, 3, 1, None) == -1
    assert L.sp_debug_blockmean_split(0, 4, 4, 1, 1, None, 0, None) == -1
    assert L.sp_debug_blockmean_split(0, 4, 4, 1, 1, None, 0, C.byref(used)) == -1 and used.value == 6
    assert L.sp_debug_blockmean_split(2, 4, 5, 1, 1, None, 0, C.byref(used)) == -1      # the run passes the width
    assert L.sp_debug_blockmean_split(0, 4, 4, 0, 1, None, 0, C.byref(used)) == -1      # no group
    assert L.sp_debug_gray_index(1.0, 0.0, 30.0, 257, None, 0, None) == -1


def test_columns_against_a_restatement(pkg):
    values = [-5, 0, 1, 2, 3, 7, 8, 63, 64, 65, 131, 1000, 2 ** 20, 2 ** 30, INT_MAX - 1, INT_MAX]
    for width in values:
        for group in values:
            assert pkg.binding.blockmean_columns(width, group) == blockmeanref.columns(width, group), (width, group)
    assert pkg.binding.blockmean_columns(INT_MAX, 1) == INT_MAX and pkg.binding.blockmean_columns(INT_MAX, INT_MAX) == 1
    assert pkg.binding.blockmean_columns(INT_MAX, INT_MAX - 1) == 2 and pkg.binding.blockmean_columns(INT_MAX, 2) == 2 ** 30


def test_host_side_block_means_as_fsum(pkg):
    plane = meanref.synthetic_plane(3, 37, 18)
    for group in (1, 2, 3, 5, 36, 37, 38, 1000):
        blockmeanref.assert_same(pkg.binding.blockmean(plane, group), blockmeanref.expected(plane, group), "synthetic, group %d" % group)
    planted = blockmeanref.planted_plane()
    blockmeanref.telling(planted)
    for group in (1, 5, 131):
        blockmeanref.assert_same(pkg.binding.blockmean(planted, group), blockmeanref.expected(planted, group), "planted, group %d" % group)
    rng = np.random.default_rng(20261021)
    for k in range(500):
        width, n, group = int(rng.integers(1, 25)), int(rng.integers(1, 5)), int(rng.integers(1, 9))
        p = meanref.random_values(rng, width * n, clustered=bool(k & 1)).reshape(width, n)
        if k % 7 == 0:
            p[int(rng.integers(0, width)), int(rng.integers(0, n))] = [math.nan, math.inf, 0.0][k % 3]
        blockmeanref.assert_same(pkg.binding.blockmean(p, group), blockmeanref.expected(p, group), "random plane %d" % k)
    assert pkg.binding.blockmean(np.zeros((0, 4)), 3).shape == (0, 4)
    with pytest.raises(pkg.SpectroplotError):
        pkg.binding.blockmean(np.array([[1.0, -1.0]]), 1)


def split_restated(x_base, frames, width, group, direct_max):
    """Frame by frame: every frame is head (its column began before the run), body (its column lies within the run) or tail."""
    head = body = tail = 0
    cols = set()
    for x in range(x_base, x_base + frames):
        c = x // group
        first, end = c * group, min((c + 1) * group, width)
        if first < x_base:
            head += 1
        elif end > x_base + frames:
            tail += 1
        else:
            body += 1
            cols.add(c)
    return {"head": head, "body": body, "tail": tail, "body_column": min(cols) if cols else None, "body_columns": len(cols),
            "direct": int(bool(cols) and group <= direct_max)}


def test_split_partitions_every_run(pkg):
    checked = 0
    for direct_max in (1, 4, 2 ** 30):
        for group in list(range(1, 13)) + [200]:
            for x_base in range(0, 41):
                for frames in range(1, 41):
                    for width in {x_base + frames, x_base + frames + 3}:
                        s = pkg.binding.blockmean_split(x_base, frames, width, group, direct_max)
                        want = split_restated(x_base, frames, width, group, direct_max)
                        what = (x_base, frames, width, group, direct_max, s)
                        assert s["head"] + s["body"] + s["tail"] == frames, what
                        assert min(s["head"], s["body"], s["tail"]) >= 0, what
                        assert (s["head"] > 0) == (x_base % group != 0), what          # a head only when a column is open
                        end = x_base + frames
                        stays_open = end % group != 0 and end != width
                        assert not s["tail"] or stays_open, what                       # a tail only when one stays open
                        if s["body"]:                                                  # body columns are whole
                            first = x_base + s["head"]
                            assert first % group == 0 and s["body_column"] == first // group, what
                            sizes = [min((c + 1) * group, width) - c * group
                                     for c in range(s["body_column"], s["body_column"] + s["body_columns"])]
                            assert sum(sizes) == s["body"] and min(sizes) >= 1, what
                        else:
                            assert s["body_columns"] == 0, what
                        for key in ("head", "body", "tail", "body_columns", "direct"):
                            assert s[key] == want[key], (key, what, want)
                        checked += 1
    assert checked > 60000
    assert pkg.binding.blockmean_split(0, 10, 10, 5, 0)["direct"] == 1     # 0: the built default


def _pattern_line(a):
    return " ".join("%x" % int(b) for b in np.ascontiguousarray(a, np.float64).view(np.uint64).reshape(-1))


def test_stand_alone_program_under_the_sanitizers_walks_planes_as_the_device_does(tmp_path):
    """csrc/sp_blockmean_core.h and csrc/sp_exact_sum.h alone, host compiler, -fsanitize=address,undefined: planes through stdin."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "blockmean_core_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes linked in: nothing has to come first at load time)
                           "-I", os.path.join(ROOT, "spectroplot-js_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "blockmean_core_check.cpp")])
    rng = np.random.default_rng(5)
    cases = []
    planted = blockmeanref.planted_plane()
    for group, direct_max in ((1, 1), (5, 1), (5, 8), (7, 2 ** 30), (64, 4), (131, 2 ** 30), (1000, 1)):
        cases.append((planted, group, direct_max, len(cases)))
    for k in range(120):
        width, n, group = int(rng.integers(1, 90)), int(rng.integers(1, 4)), int(rng.integers(1, 20))
        p = meanref.random_values(rng, width * n, clustered=bool(k & 1)).reshape(width, n)
        if k % 5 == 0:
            p[int(rng.integers(0, width)), int(rng.integers(0, n))] = [math.nan, math.inf][k % 2]
        cases.append((p, group, [1, 4, 2 ** 30][k % 3], k))
    text = "".join("%d %d %d %d %d\n%s\n" % (p.shape[1], p.shape[0], group, dm, seed, _pattern_line(p)) for p, group, dm, seed in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split("\n")
    assert len(lines) == len(cases) + 1 and lines[-1] == ""
    for (p, group, dm, seed), line in zip(cases, lines):
        assert line not in ("mismatch", "broken split"), (line, p.shape, group, dm)
        got = np.array([int(w, 16) for w in line.split()], np.uint64).view(np.float64).reshape(-1, p.shape[1])
        blockmeanref.assert_same(got, blockmeanref.expected(p, group), "plane %r, group %d, direct_max %d" % (p.shape, group, dm))


@pytest.mark.parametrize("ps", [edgeref.SWEEP[6], edgeref.SWEEP[8], edgeref.DEFAULT], ids=lambda ps: "lut_%d" % ps.lut_len)
def test_colour_index_two_ulps_either_side_of_every_edge(pkg, ps):
    assert ps.lut_len in (2, 17, 256)
    scales = edgeref.Scales(ps.gain, ps.rng, ps.lut_len, ps.block_norm)
    edges, _ = edgeref.index_edges(ps.gain, ps.rng, ps.lut_len, ps.block_norm)
    assert len(edges) == ps.lut_len - 1                                       # every colour step is reachable with these parameters
    values = (edges.view(np.int64)[:, None] + np.arange(-2, 3, dtype=np.int64)[None, :]).view(np.float64).reshape(-1)
    want = np.array([scales.gray(float(v)) for v in values])
    assert set(want) == set(range(ps.lut_len))                                # both sides of every edge are there
    got = pkg.binding.gray_index(ps.block_norm, ps.gain, ps.rng, ps.lut_len, values)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    specials = np.array([0.0, math.inf, math.nan, 5e-324, float(np.finfo(np.float64).max)])
    got = pkg.binding.gray_index(ps.block_norm, ps.gain, ps.rng, ps.lut_len, specials)
    assert list(got) == [0, ps.lut_len - 1, 0, 0, ps.lut_len - 1]
