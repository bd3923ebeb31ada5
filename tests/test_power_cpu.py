"""Power plane replies without a device: the expected-plane construction the GPU tests use (tests/powerref.py) against the reference the
traces are pinned to, the ABI, and the compiled k_frames_power variants with their register / spill table."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import isa
import powerref
import siggen
import tracesref
from __graft_entry__ import ROOT, build, load_package
from test_traces_cpu import SHAPES, _variants

GEN = {"kind": "trinoise", "seed": 4711, "step": 4099, "gshift": 9, "amp": 0.45, "namp": 0.03}
ENTRY_POINTS = ("sp_plan_execute_power", "sp_plan_power_to_db", "sp_render_power", "sp_plan_power_kernel_name_for")
MANGLED = "_ZN4spk214k_frames_power"


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def power_objs():
    objs = sorted(glob.glob(os.path.join(isa.PKG, "build", "power_*.o")))
    if len(objs) < 5:
        build()
        objs = sorted(glob.glob(os.path.join(isa.PKG, "build", "power_*.o")))
    assert len(objs) == 5
    return objs


def _objs(pattern):
    return sorted(glob.glob(os.path.join(isa.PKG, "build", pattern)))


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    for decl in ("int sp_plan_execute_power(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_power);",
                 "int sp_plan_power_to_db(sp_plan *plan, const double *d_power, size_t count, double *d_db);",
                 "int sp_render_power(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db, "
                 "double *power);",
                 "const char *sp_plan_power_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);"):
        assert decl in hdr, decl
    text = hdr[hdr.index("Power plane replies"):hdr.index("int sp_plan_execute_power(")]
    for word in ("SP_ERR_UNSUPPORTED", "NaN", "worker.js:90", "Out of scope"):
        assert word in text, word
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for name in ("execute_power", "power_to_db", "power_kernel_name_for"):
        assert hasattr(pkg.Plan, name), name
    assert hasattr(pkg.Context, "render_power")
    # no existing structure changed
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.DETECTORS == {"sample": 0, "peak": 1}


def test_null_plan_is_an_invalid_argument(pkg):
    L = pkg.Library.get().L
    assert L.sp_plan_execute_power(None, None, 0, 0, None) == -1
    assert L.sp_plan_power_to_db(None, None, 0, None) == -1
    assert L.sp_render_power(None, None, None, 0, 0, 0, None) == -1
    assert L.sp_plan_power_kernel_name_for(None, 0, 0) == b""


@pytest.mark.parametrize("fmt,n,width,samples,ch", SHAPES)
def test_reference_planes_fold_to_the_reference_traces(fmt, n, width, samples, ch):
    """The dB plane folded along x with the traces' own fold is the traces' reference, bit for bit, and the power plane is the abs2 plane
    in row order: the planes are pinned to what the traces are pinned to."""
    data = siggen.generate(fmt, GEN, samples)
    win, weight = powerref.pyoracle.window("hann", n)
    want = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 40.0, width, ch)
    assert want["power"].shape == (width, n) and want["db"].shape == (width, n)
    traces = tracesref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 40.0, width, ch)
    tmin, tmax = tracesref.fold(want["db"])          # (the fold is per column: it commutes with the row permutation)
    assert tracesref.same_bits(tmin, traces["trace_min"]) and tracesref.same_bits(tmax, traces["trace_max"])
    y = tracesref.rows(n)
    assert powerref.same_plane(want["power"][:, y], want["ref"]["abs2"])
    assert not np.signbit(want["power"][~np.isnan(want["power"])]).any()          # |X|^2 is never -0


def test_same_plane_leaves_only_the_kind_of_nan_uncompared():
    a = np.array([[1.0, np.nan, 0.0, np.inf]])
    other_nan = np.frombuffer(np.array([0xfff8000000000123], np.uint64).tobytes(), np.float64)[0]
    assert powerref.same_plane(a, np.array([[1.0, other_nan, 0.0, np.inf]]))
    assert not powerref.same_plane(a, np.array([[1.0, np.nan, -0.0, np.inf]]))
    assert not powerref.same_plane(a, np.array([[1.0, 2.0, 0.0, np.inf]]))
    assert not powerref.same_plane(a, np.array([[np.nan, np.nan, 0.0, np.inf]]))
    assert not powerref.same_plane(a, np.array([[np.nextafter(1.0, 2.0), np.nan, 0.0, np.inf]]))
    assert not powerref.same_plane(a, a.reshape(4, 1))
    assert powerref.same_plane(np.zeros((0, 8)), np.zeros((0, 8)))


def test_power_objects_hold_only_k_frames_power_and_nobody_else_does():
    for o in power_objs():
        names = re.findall(r"\.name:\s*(\S+)", isa.notes(o))
        kernels = [k for k in names if not k.endswith(".kd")]
        assert kernels and all(k.startswith(MANGLED + "I") for k in kernels), (o, kernels[:3])
    others = _objs("frames_*.o") + _objs("peak_*.o") + _objs("traces_*.o") + _objs("index_*.o")
    assert len(others) == 8 + 5 + 5 + 8
    for o in others + [os.path.join(isa.PKG, "build", "sp_kernels.o")]:
        assert "k_frames_power" not in isa.notes(o), o


def test_all_sixty_variants_exist_and_the_prefetching_iq_ones_use_no_scratch():
    seen = _variants(power_objs(), MANGLED)
    assert sorted(seen) == sorted((lg, ch, p) for lg in range(6, 11) for ch in (False, True) for p in (0, 1, 2, 3, 4, 8))
    for (lg, ch, p), (vgpr, spill, priv) in seen.items():
        if not ch and p:
            assert priv == 0 and spill == 0, ((lg, ch, p), priv, spill)


def test_design_table_is_what_the_objects_say():
    """DESIGN.md section 15 lists VGPRs / spilled VGPRs per (n, I/Q or L/R) for the loaders 1, 2, 3, 4, 8 bytes and the generic one."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 15."):]
    table = {}
    for m in re.finditer(r"^\| (\d+) points \| (I/Q|L/R) \|((?: \d+ / \d+ \|){6})\s*$", sec, re.M):
        cells = [tuple(int(v) for v in c.split("/")) for c in m.group(3).strip(" |").split("|")]
        table[(int(m.group(1)).bit_length() - 1, m.group(2) == "L/R")] = cells
    assert sorted(table) == sorted((lg, ch) for lg in range(6, 11) for ch in (False, True))
    seen = _variants(power_objs(), MANGLED)
    for (lg, ch, p), (vgpr, spill, priv) in seen.items():
        assert table[(lg, ch)][(1, 2, 3, 4, 8, 0).index(p)] == (vgpr, spill), ((lg, ch, p), (vgpr, spill))
