"""Indexed image replies without a device: the ABI, the compiled k_frames_index variants against k_frames' under the register rule of
sp_kernel_frames.h, their register / spill table in DESIGN.md section 13, and the lattice of the GPU test."""
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess

import numpy as np

import pytest

import indexref
import isa
import launchref
from __graft_entry__ import ROOT, build, load_package
from test_traces_cpu import _variants

ENTRY_POINTS = ("sp_context_last_chunks", "sp_plan_execute_index", "sp_render_index", "sp_index_to_rgba", "sp_plan_index_kernel_name_for", "sp_plan_debug_index_launch")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def index_objs():
    objs = sorted(glob.glob(os.path.join(isa.PKG, "build", "index_*.o")))
    if len(objs) < 8:
        build()
        objs = sorted(glob.glob(os.path.join(isa.PKG, "build", "index_*.o")))
    assert len(objs) == 8
    return objs


def test_header_declares_and_library_exports_and_binds_the_entry_points(pkg):
    hdr = open(os.path.join(ROOT, "include", "spectroplot_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
    sec = hdr[hdr.index("Indexed image replies"):hdr.index("int sp_plan_execute_index(")]
    assert "SP_ERR_UNSUPPORTED" in sec and "SP_ERR_INVALID_ARG" in sec and "(0, 0, 0, 255)" in sec and "Out of scope" in sec
    L = C.CDLL(pkg.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    for cls, names in ((pkg.Plan, ("execute_index", "index_kernel_name_for", "debug_index_launch")), (pkg.Context, ("render_index", "index_to_rgba"))):
        for name in names:
            assert hasattr(cls, name), name
    b = pkg.binding
    assert C.sizeof(b._Request) == 64 and C.sizeof(b._Reply) == 56     # no existing structure changed


def test_entry_points_without_a_context_or_plan(pkg):
    """No object to work on: SP_ERR_NO_DEVICE without a device (there is no CPU path), SP_ERR_INVALID_ARG with one."""
    L = C.CDLL(pkg.lib_path())
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
    L.sp_plan_execute_index.argtypes = [vp, vp, sz, i32, vp, vp]
    L.sp_render_index.argtypes = [vp, vp, vp, sz, i32, vp, vp]
    L.sp_index_to_rgba.argtypes = [vp, vp, sz, vp, i32, vp]
    L.sp_plan_index_kernel_name_for.restype = C.c_char_p
    L.sp_plan_index_kernel_name_for.argtypes = [vp, sz, i32]
    want = -5 if pkg.Library.get().device_count() == 0 else -1
    assert L.sp_plan_execute_index(None, None, 0, 0, None, None) == want
    assert L.sp_render_index(None, None, None, 0, 0, None, None) == want
    assert L.sp_index_to_rgba(None, None, 0, None, 0, None) == want
    assert L.sp_plan_index_kernel_name_for(None, 0, 0) == b""


def test_index_objects_hold_only_k_frames_index_and_nobody_else_does():
    for o in index_objs():
        names = re.findall(r"\.name:\s*(\S+)", isa.notes(o))
        kernels = [k for k in names if not k.endswith(".kd")]
        assert kernels and all(k.startswith("_ZN4spk214k_frames_indexI") for k in kernels), (o, kernels[:3])
    for o in isa.frame_objs() + isa.peak_objs():
        assert "k_frames_index" not in isa.notes(o), o


def test_every_variant_meets_the_register_rule_against_k_frames(pkg):
    """A variant exists only if it spills no more VGPRs than the k_frames variant of the same (n, L/R, loader): the objects hold exactly
    the variants of frames_index_variant_built (restated as indexref.built), each within its twin's spill count, and no prefetching I/Q
    variant spills."""
    mine = _variants(index_objs(), "_ZN4spk214k_frames_index")
    theirs = _variants(isa.frame_objs(), "_ZN4spk28k_frames")
    assert sorted(mine) == sorted(k for k in theirs if indexref.built(1 << k[0], k[2], k[1])) and len(mine) == 93
    for (lg, ch, p), (vgpr, spill, priv) in mine.items():
        assert spill <= theirs[(lg, ch, p)][1], ((lg, ch, p), spill, theirs[(lg, ch, p)][1])
        if not ch and p:
            assert spill == 0, ((lg, ch, p), spill)
            # an open point of DESIGN.md section 13, pinned so that a growth is noticed: the n = 1024 variants declare a private
            # segment of 36 bytes that no instruction of theirs addresses (the next test); every other size declares none
            assert priv == (36 if lg == 10 else 0), ((lg, ch, p), priv)


def test_the_prefetching_iq_variants_issue_no_scratch_instruction():
    c = isa.checker()
    seen = 0
    for o in index_objs():
        cur = None
        for ln in c.disassemble(o):
            h = re.match(r"^[0-9a-f]+ <_ZN4spk214k_frames_indexILi(\d+)ELb([01])ELi(\d+)E", ln)
            if h:
                cur = h.groups() if h.group(2) == "0" and h.group(3) != "0" else None
                seen += cur is not None
                continue
            if re.match(r"^[0-9a-f]+ <", ln):
                cur = None
            if cur:
                assert not re.search(r"\s(scratch_|buffer_)(load|store)", ln), (cur, ln)
    assert seen == 8 * 5


def test_design_table_is_what_the_objects_say():
    """DESIGN.md section 13 lists VGPRs / spilled VGPRs per (n, I/Q or L/R) for the loaders 1, 2, 3, 4, 8 bytes and the generic one
    (rows `| n = 64 | I/Q | ...`: section 12's rows start with the bare number)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 13."):]
    table = {}
    for m in re.finditer(r"^\| n = (\d+) \| (I/Q|L/R) \|((?: \d+ / \d+ \|){6})\s*$", sec, re.M):
        cells = [tuple(int(v) for v in c.split("/")) for c in m.group(3).strip(" |").split("|")]
        table[(int(m.group(1)).bit_length() - 1, m.group(2) == "L/R")] = cells
    assert sorted(table) == sorted((lg, ch) for lg in range(6, 14) for ch in (False, True))
    seen = _variants(index_objs(), "_ZN4spk214k_frames_index")
    for (lg, ch, p), (vgpr, spill, priv) in seen.items():
        assert table[(lg, ch)][(1, 2, 3, 4, 8, 0).index(p)] == (vgpr, spill), ((lg, ch, p), (vgpr, spill))
    for (lg, ch), cells in table.items():                               # a variant that is not built: `0 / 0`
        assert all(cells[(1, 2, 3, 4, 8, 0).index(p)] == (0, 0) for p in (1, 2, 3, 4, 8, 0) if (lg, ch, p) not in seen), (lg, ch)


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_recolour_is_numpys_take_on_the_golden_colour_maps(tmp_path):
    """js/consumers.js recolour(index, cmap) == take(cmap, index) with alpha 255, and (0, 0, 0, 255) for an index the map does not have,
    for every map of tests/golden/cmaps.bin whole and cut to 100 entries (tests/js/check_recolour.js)."""
    gdir = os.path.join(ROOT, "tests", "golden")
    meta = json.load(open(os.path.join(gdir, "cmaps.json")))
    cbin = np.fromfile(os.path.join(gdir, "cmaps.bin"), dtype=np.uint8)
    index = ((np.arange(5003) * 37 + 11) & 255).astype(np.uint8)
    assert len(np.unique(index)) == 256
    index.tofile(str(tmp_path / "index.bin"))
    for e in meta:
        for length in (e["length"], 100):
            table = np.zeros((256, 4), np.uint8)
            table[:, 3] = 255
            table[:length, :3] = cbin[e["offset"]:e["offset"] + 3 * length].reshape(-1, 3)
            np.take(table, index, axis=0).tofile(str(tmp_path / ("%s_%d.rgba" % (e["name"], length))))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_recolour.js"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "recolour checks ok: %d" % (4 * len(meta)) in out.stdout


def test_the_gpu_lattice_covers_what_it_claims():
    cases = indexref.lattice()
    assert len(cases) == 48 and len({indexref.case_id(c) for c in cases}) == 48
    assert {(c["n"], c["loader"]) for c in cases} == {(n, p) for n in launchref.SIZES for p in launchref.LOADERS}
    assert all(indexref.built(c["n"], c["loader"], c["ch"]) for c in cases)
    assert any(c["n"] == 1024 and c["gf"] == 32 and launchref.halves(c["n"], c["gf"]) for c in cases)
    for n in launchref.SIZES:
        gfs = launchref.reachable_gf(n)
        cells = {(c["gf"], c["regime"]) for c in cases if c["n"] == n}
        assert cells >= {(gfs[0], "mixed"), (gfs[0], "many")} | {(gf, "many") for gf in gfs[1:]}, (n, cells)
    assert {c["writeout"] for c in cases} == {"fast", "w4", "w1", "p1", "p4"}
    for cu in (256, 304, 64):
        for c in cases:
            W = indexref.choose_width(c["n"], cu, c["gf"], c["regime"], c["writeout"])
            assert W is not None and indexref.width_ok(W, c["writeout"]) and W * c["n"] <= 128 << 20, (cu, c)
