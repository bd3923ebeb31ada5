"""The launch shapes of the portable ("scratch") kernels without a device: tests/scratchref.py's restatement against the library's own
functions (sp_debug_scratch_launch calls scratch_blocks, which every scratch launch sizes its grid with, and scratch_wide, which
dispatch_scratch picks the variant with); the stages per barrier of the four-stage frame; and what the cases of
tests/test_scratch_shapes_gpu.py cover."""
import ctypes as C
import os

import pytest

import scratchref
from __graft_entry__ import build, load_package

SIZES = [1 << k for k in range(1, 21)]                  # n = 2 .. SP_MAX_N
FRAMES = (1, 2, 1023, 1024, 1025, 5000)
CUS = (1, 8, 32, 64, 256, 304)


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def test_restated_shape_equals_the_librarys(pkg):
    sl = pkg.binding.debug_scratch_launch
    assert sorted(set(scratchref.SLABS.values())) == [2, 3, 4] and scratchref.SLABS == {"image": 2, "peak": 3, "traces": 4, "power": 2}
    seen = set()
    for n in SIZES:
        for slabs in (2, 3, 4):
            for frames in FRAMES:
                for cu in CUS:
                    got, want = sl(n, slabs, frames, cu), (scratchref.workgroups(n, slabs, frames, cu), scratchref.wide(n))
                    assert got == want, (n, slabs, frames, cu, got, want)
                    assert 1 <= got[0] <= frames and got[0] * 8 * slabs * n <= max(scratchref.CAP_BYTES, 8 * slabs * n)
                    seen.add("frames" if got[0] == frames else "part" if got[0] == 4 * cu else "cap")
    assert seen == {"frames", "part", "cap"}             # each of the three bounds is the one that holds somewhere
    assert [n for n in SIZES if scratchref.wide(n)][0] == 4096
    # the issue's figures: 16 workgroups of an image or of traces, 10 of a held peak
    assert sl(1 << 20, 2, 19, 256)[0] == 16 and sl(1 << 19, 4, 35, 256)[0] == 16 and sl(1 << 20, 3, 11, 256)[0] == 10


def test_debug_entry_checks_its_arguments(pkg):
    lib = C.CDLL(pkg.lib_path())
    lib.sp_debug_scratch_launch.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    out, used = (C.c_int64 * 2)(), C.c_size_t()
    assert lib.sp_debug_scratch_launch(4096, 2, 10, 256, out, 2, C.byref(used)) == 0 and used.value == 2 and list(out) == [10, 1]
    assert lib.sp_debug_scratch_launch(4096, 2, 10, 256, out, 1, C.byref(used)) == -1 and used.value == 2      # capacity
    assert lib.sp_debug_scratch_launch(4096, 2, 10, 256, None, 2, C.byref(used)) == -1
    assert lib.sp_debug_scratch_launch(4096, 2, 10, 256, out, 2, None) == -1
    for bad in ((1, 2, 10, 256), (100, 2, 10, 256), (1 << 21, 2, 10, 256), (64, 0, 10, 256), (64, 2, 0, 256), (64, 2, 10, 0)):
        assert lib.sp_debug_scratch_launch(*bad, out, 2, C.byref(used)) == -1, bad


def test_stage_groups():
    table = {12: [4, 4, 4], 13: [4, 4, 4, 1], 14: [4, 4, 4, 2], 15: [4, 4, 4, 3], 19: [4, 4, 4, 4, 3], 20: [4, 4, 4, 4, 4]}
    for levels, groups in table.items():
        assert scratchref.stage_groups(levels) == groups, levels
    for levels in range(12, 21):
        g = scratchref.stage_groups(levels)
        assert sum(g) == levels and all(v == 4 for v in g[:-1]) and 1 <= g[-1] <= 4
        assert scratchref.wide(1 << levels)


def test_columns_of():
    for frames, groups in ((1, 1), (5, 3), (19, 16), (2053, 1024), (1024, 1024)):
        cols = [scratchref.columns_of(b, frames, groups) for b in range(groups)]
        assert sorted(x for c in cols for x in c) == list(range(frames))
        assert all(c == sorted(c) and all(x % groups == b for x in c) for b, c in enumerate(cols))
        assert max(len(c) for c in cols) == -(-frames // groups)


def test_what_the_gpu_cases_cover():
    import test_scratch_shapes_gpu as gpu
    assert gpu.last_groups() == {1, 2, 3, 4}
    assert len({c["id"] for c in gpu.CASES}) == len(gpu.CASES)
    by_part = {p: [c for c in gpu.CASES if c["part"] == p] for p in ("B1", "B2", "B3")}
    for cu in CUS[1:]:
        for c in by_part["B1"] + by_part["B3"]:
            W, B = gpu._shape(c, cu)
            assert B < W, (c["id"], cu)
            if c["part"] == "B3":
                assert B in (10, 16) and B < 4 * cu
    for n in (1 << 15, 1 << 19, 1 << 20):
        assert {c["kind"] for c in by_part["B2"] if c["n"] == n} == {"image", "peak", "traces", "power"}
    assert {c["ch"] for c in by_part["B2"] if c["n"] == 1 << 20} == {False, True}
    assert {c["fmt"] for c in by_part["B2"]} >= {"CF32", "CS12", "CU8"} and {c["wf"] for c in by_part["B2"]} == {False, True}
    assert any(c["oob"] and c["n"] == 1 << 19 for c in by_part["B2"])
    assert {(c["kind"], c["n"]) for c in by_part["B1"]} == {("image", 32), ("image", 4096), ("peak", 32), ("peak", 4096), ("traces", 2048),
                                                            ("traces", 4096), ("power", 2048), ("power", 4096)}


def test_what_the_cu_count_cases_cover(pkg):
    """tests/test_cu_counts_gpu.py, part D: on 8 CUs the part is the bound - 32 workgroups for 100 frames, three or four columns each -
    for every kind at n = 32, 2048, 8192 and 16384, through both variants."""
    import test_cu_counts_gpu as gpu
    assert gpu.SCRATCH_CU == 8 and len({c["id"] for c in gpu.D_CASES}) == len(gpu.D_CASES) == 16
    assert {(c["kind"], c["n"]) for c in gpu.D_CASES} == {(k, n) for k in scratchref.SLABS for n in (32, 2048, 8192, 16384)}
    for c in gpu.D_CASES:
        W, B = gpu.ss._shape(c, 8)
        assert (W, B) == (100, 32) and pkg.binding.debug_scratch_launch(c["n"], scratchref.SLABS[c["kind"]], W, 8) == (32, c["n"] >= 4096)
        assert sorted({len(scratchref.columns_of(b, W, B)) for b in range(B)}) == [3, 4]
        assert c["force"] == (c["n"] in (2048, 8192))
    assert {c["ch"] for c in gpu.D_CASES} == {False, True} and {c["fmt"] for c in gpu.D_CASES} == {"CS16", "CU8", "CF32", "CS12"}
