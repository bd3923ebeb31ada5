"""The lattice of tests/variantref.py without a device: it is the set of frame-loop kernels in the built objects, family by family, and
every cell's request reaches the cell - the launch shape through the library's own rule, the loader through frames_prefetch_width
restated (variantref.prefetch_width) and, for the batch cells, through the library's own work list (sp_debug_batch_plan)."""
import glob
import os
import re

import pytest

import isa
import launchref
import siggen
import variantref
from __graft_entry__ import build, load_package

CELLS = variantref.lattice()


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def _objs(pattern):
    objs = sorted(glob.glob(os.path.join(isa.PKG, "build", pattern)))
    if not objs:
        build()
        objs = sorted(glob.glob(os.path.join(isa.PKG, "build", pattern)))
    return objs


def _compiled(family):
    """{(log2n, L/R, loader)} of the family's kernels in the built objects."""
    seen = set()
    for o in _objs(variantref.OBJECTS[family]):
        for blk in isa.notes(o).split(".name:")[1:]:
            m = re.match(r"\s*" + variantref.mangled(family) + r"Li(\d+)ELb([01])ELi(\d+)EEEv", blk)
            if m and not blk.split()[0].endswith(".kd"):
                seen.add((int(m.group(1)), m.group(2) == "1", int(m.group(3))))
    return seen


@pytest.mark.parametrize("family", list(variantref.FAMILIES))
def test_the_lattice_is_the_set_of_compiled_kernels(family):
    """A variant added later (or one that is no longer built) fails here until the lattice, and with it the GPU cases, follow."""
    want = variantref.variants(family)
    assert len(want) == len(set(want)) == variantref.COUNTS[family]
    got = _compiled(family)
    assert got == set(want), (family, sorted(got - set(want))[:6], sorted(set(want) - got)[:6])


def test_no_other_frame_loop_kernel_is_compiled():
    """Every kernel of the per-n objects belongs to one of the six families: 417 in all."""
    names = set()
    for pattern in sorted(set(variantref.OBJECTS.values())):
        for o in _objs(pattern):
            names |= {k for k in re.findall(r"\.name:\s*(\S+)", isa.notes(o)) if not k.endswith(".kd")}
    starts = tuple(variantref.mangled(f) + "Li" for f in variantref.FAMILIES)
    assert all(k.startswith(starts) for k in names), sorted(k for k in names if not k.startswith(starts))[:4]
    assert len(names) == sum(variantref.COUNTS.values()) == 417


def test_one_cell_per_variant_and_what_rotates():
    assert len(CELLS) == 417 and len({variantref.case_id(c) for c in CELLS}) == 417
    for family in variantref.FAMILIES:
        mine = [c for c in CELLS if c["family"] == family]
        assert sorted((c["n"].bit_length() - 1, c["ch"], c["loader"]) for c in mine) == sorted(variantref.variants(family))
        if family in ("frames", "peak", "index", "batch"):
            assert {c["wf"] for c in mine} == {False, True}
        if family in ("frames", "peak", "index"):
            assert {variantref.is_fast(c) for c in mine} == {False, True}, family
            assert {(c["loader"], variantref.is_fast(c)) for c in mine} == {(p, f) for p in variantref.LOADERS for f in (False, True)}, family
        generic = [c["fmt"] for c in mine if c["loader"] == 0]
        assert set(generic) == set(variantref.GENERIC_FORMATS) and all(siggen.SAMPLE_WIDTH[f] == 16 for f in generic)
        for c in mine:
            if c["loader"]:
                assert c["fmt"] in launchref.LOADER_FORMATS[c["loader"]] and siggen.SAMPLE_WIDTH[c["fmt"]] == c["loader"]
    assert {c["M"] for c in CELLS if c["family"] == "peak"} == {2, 3}


def test_the_deal_of_nineteen_groups_on_eight_cus():
    grid = launchref.grid_for(variantref.GROUPS, variantref.CU)
    assert grid == 8 and launchref.deal(variantref.GROUPS, grid) == [3, 3, 3, 3, 3, 3, 1, 0]


@pytest.mark.parametrize("k", range(len(CELLS)), ids=[variantref.case_id(c) for c in CELLS])
def test_the_request_reaches_its_cell(pkg, k):
    c = CELLS[k]
    n, gf, cu = c["n"], variantref.gf_of(c["n"]), variantref.CU
    reqs = variantref.requests(c)
    sw = siggen.SAMPLE_WIDTH[c["fmt"]]
    if c["family"] == "batch":
        widths = [W for W, _, _ in reqs]
        assert widths == [gf + 1, 1, (variantref.GROUPS - 3) * gf - 1] and widths[2] % gf != 0
        pgf, grids, groups, rows = pkg.binding.debug_batch_plan(c["fmt"], n, 256, cu, [nb for _, _, nb in reqs], widths)
        launches = [int(r[0]) for r in rows]
        assert pgf == gf == launchref.batch_gf(n, sum(widths), cu) and sum(groups) == variantref.GROUPS
        assert launches == variantref.batch_launches(c) == ([1, 1, 1] if c["loader"] == 0 else [0, 1, 0] if sw == 3 else [0, 0, 0]), (launches, rows)
        assert [int(r[2]) for r in rows] == [2, 1, variantref.GROUPS - 3]
        # the launch that holds the large ragged item is the cell's: its loader is the format's, or the generic one
        assert variantref.prefetch_width(c["fmt"], n, reqs[2][2], widths[2]) == c["loader"]
        return
    (W, samples, nbytes), = reqs
    assert nbytes == samples * sw and nbytes <= 8 << 20
    assert pkg.binding.debug_frames_launch(n, 256, W, cu)[:3] == launchref.launch(n, 256, W, cu) == (gf, variantref.GROUPS, 8)
    assert W % gf != 0 and W >= 2
    assert variantref.prefetch_width(c["fmt"], n, nbytes, W) == c["loader"]
    last = variantref.frame_start(samples, n, W, W - 1)
    assert last >= 1 and last + n <= samples
    if c["family"] == "peak":
        assert pkg.binding.peak_subframes(c["fmt"], n, nbytes, W) == (c["M"], 1)
        assert (samples - n) / (W - 1) >= 2 * n
    else:
        assert (samples - n) / (W - 1) == variantref.hop(n) and variantref.hop(n) % 2 == 1      # overlapping frames, unaligned starts
