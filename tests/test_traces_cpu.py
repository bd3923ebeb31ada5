"""Per-bin min / max traces without a device: the expected-value construction the GPU tests use (tests/tracesref.py) against the
identity it must satisfy, the ABI, and the compiled k_frames_traces variants with their register / spill table."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import isa
import siggen
import tracesref
from __graft_entry__ import ROOT, build, load_package
from oracle import pyoracle

GEN = {"kind": "trinoise", "seed": 4711, "step": 4099, "gshift": 9, "amp": 0.45, "namp": 0.03}
ENTRY_POINTS = ("sp_plan_execute_traces", "sp_render_traces", "sp_plan_traces_kernel_name_for")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def traces_objs():
    objs = sorted(glob.glob(os.path.join(isa.PKG, "build", "traces_*.o")))
    if len(objs) < 5:
        build()
        objs = sorted(glob.glob(os.path.join(isa.PKG, "build", "traces_*.o")))
    assert len(objs) == 5
    return objs


# (format, n, width, samples, L/R split)
SHAPES = [
    ("CU8", 4, 5, 40, False), ("CU8", 16, 9, 300, False), ("CS8", 32, 1, 100, True), ("CS16", 64, 37, 64 + 36 * 100, False),
    ("CF32", 128, 21, 128 + 20 * 255, True), ("CS12", 64, 9, 300, False), ("CU12", 256, 12, 256 + 11 * 256, True),
    ("CF64", 64, 30, 64 + 29 * 31, False), ("CU4", 128, 20, 128 * 20, False), ("CS32", 512, 6, 512 * 4, True),
    ("CU16", 1024, 5, 1024 * 3, False), ("CS64", 2048, 3, 2048 * 2 + 17, False),
]


@pytest.mark.parametrize("fmt,n,width,samples,ch", SHAPES)
def test_reference_traces_fold_to_the_oracles_dbfs_range(fmt, n, width, samples, ch):
    data = siggen.generate(fmt, GEN, samples)
    win, weight = pyoracle.window("hann", n)
    want = tracesref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 40.0, width, ch)
    assert want["trace_min"].shape == (n,) and want["trace_max"].shape == (n,)
    assert tracesref.same_bits(want["trace_min"].min(), want["dBfs_min"])
    assert tracesref.same_bits(want["trace_max"].max(), want["dBfs_max"])
    # both layouts read the same arrays: row y of the spectrogram is bin i of worker.js:90
    ref = pyoracle.render(fmt, data, n, win, 1.0 / weight, 3.0, 40.0, tracesref._LUT, width, ch, False, planes=True)
    y = tracesref.rows(n)
    assert sorted(y.tolist()) == list(range(n))
    with np.errstate(invalid="ignore"):
        assert tracesref.same_bits(want["trace_max"][y], np.fmax.reduce(np.vstack([ref["db"], np.full((1, n), -200.0)]), axis=0))


def test_reference_fold_ignores_nan_and_keeps_the_start_values():
    db = np.array([[np.nan, -3.0, np.nan, -np.inf], [np.nan, -250.0, 5.0, np.nan]])
    tmin, tmax = tracesref.fold(db)
    assert tmin.tolist() == [0.0, -250.0, 0.0, -np.inf] and tmax.tolist() == [-200.0, -3.0, 5.0, -200.0]
    tmin, tmax = tracesref.fold(np.zeros((0, 3)))
    assert tmin.tolist() == [0.0] * 3 and tmax.tolist() == [-200.0] * 3


def test_header_declares_and_library_exports_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    assert re.search(r"int sp_plan_execute_traces\(sp_plan \*plan, const void \*d_bytes, size_t nbytes, int32_t width, double \*d_trace_min,\s*"
                     r"double \*d_trace_max\);", hdr)
    assert re.search(r"int sp_render_traces\(sp_context \*ctx, const sp_request \*req, const uint8_t \*bytes, size_t nbytes, int32_t width,\s*"
                     r"double \*trace_min,\s*double \*trace_max\);", hdr)
    assert "const char *sp_plan_traces_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);" in hdr
    assert "SP_ERR_UNSUPPORTED" in hdr[hdr.index("Per-bin min / max traces"):hdr.index("int sp_plan_execute_traces(")]
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    assert hasattr(pkg.Plan, "execute_traces") and hasattr(pkg.Plan, "traces_kernel_name_for") and hasattr(pkg.Context, "render_traces")
    # no existing structure changed
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56 and b.DETECTORS == {"sample": 0, "peak": 1}


def _variants(objs, mangled):
    """{(log2n, L/R, loader): (vgprs, spilled vgprs, private bytes)} of the kernels whose mangled name starts with `mangled`."""
    seen = {}
    for o in objs:
        for blk in isa.notes(o).split(".name:")[1:]:
            m = re.match(r"\s*" + mangled + r"ILi(\d+)ELb([01])ELi(\d+)E", blk)
            if not m:
                continue
            priv = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
            spill = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1))
            vgpr = int(re.search(r"\.vgpr_count:\s*(\d+)", blk).group(1))
            seen[(int(m.group(1)), m.group(2) == "1", int(m.group(3)))] = (vgpr, spill, priv)
    return seen


def test_traces_objects_hold_only_k_frames_traces_and_nobody_else_does():
    objs = traces_objs()
    for o in objs:
        names = re.findall(r"\.name:\s*(\S+)", isa.notes(o))
        kernels = [k for k in names if not k.endswith(".kd")]
        assert kernels and all(k.startswith("_ZN4spk215k_frames_tracesI") for k in kernels), (o, kernels[:3])
    others = isa.frame_objs() + isa.peak_objs() + [os.path.join(isa.PKG, "build", "sp_kernels.o")]      # every other object with kernels
    for o in others:
        assert "k_frames_traces" not in isa.notes(o), o


def test_all_sixty_variants_exist_and_the_prefetching_iq_ones_use_no_scratch():
    seen = _variants(traces_objs(), "_ZN4spk215k_frames_traces")
    assert sorted(seen) == sorted((lg, ch, p) for lg in range(6, 11) for ch in (False, True) for p in (0, 1, 2, 3, 4, 8))
    for (lg, ch, p), (vgpr, spill, priv) in seen.items():
        if not ch and p:
            assert priv == 0 and spill == 0, ((lg, ch, p), priv, spill)


def test_design_table_is_what_the_objects_say():
    """DESIGN.md section 12 lists VGPRs / spilled VGPRs per (n, I/Q or L/R) for the loaders 1, 2, 3, 4, 8 bytes and the generic one."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 12."):]
    table = {}
    for m in re.finditer(r"^\| (\d+) \| (I/Q|L/R) \|((?: \d+ / \d+ \|){6})\s*$", sec, re.M):
        cells = [tuple(int(v) for v in c.split("/")) for c in m.group(3).strip(" |").split("|")]
        table[(int(m.group(1)).bit_length() - 1, m.group(2) == "L/R")] = cells
    assert sorted(table) == sorted((lg, ch) for lg in range(6, 11) for ch in (False, True))
    seen = _variants(traces_objs(), "_ZN4spk215k_frames_traces")
    for (lg, ch, p), (vgpr, spill, priv) in seen.items():
        assert table[(lg, ch)][(1, 2, 3, 4, 8, 0).index(p)] == (vgpr, spill), ((lg, ch, p), (vgpr, spill))
