"""The launch shapes of the frame-loop kernels without a device: tests/launchref.py's restatement of the launch rule against the
library's own (sp_debug_frames_launch calls frames_launch_rule, the function every launch of k_frames, k_frames_peak and k_frames_batch
goes through), for every n the kernels take; the width chooser against the restatement; and what the lattice of
tests/test_launch_shapes_gpu.py covers."""
import ctypes as C
import itertools
import os

import pytest

import launchref
from __graft_entry__ import build, load_package

CUS = (8, 16, 20, 24, 32, 64, 104, 128, 256, 304)
SHORT = (8, 20)                                    # the counts at which 3 * grid + 7 groups are more than a gf below the largest is kept for


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


def _threshold_counts(cu):
    """Frame counts on both sides of and on every point where the rule changes its mind: the three thresholds of `want`, the grid's
    steps around the CU count, the smallest launches."""
    out = set(range(1, 40))
    for w in (4, 8, 16, 32):
        t = w * (2 * cu - 1)                       # the last count whose ceil(count / w) is below 2 * cu
        out.update((t - 1, t, t + 1, t + 2, t + w, 2 * t, 2 * t + 1))
    for gf in (4, 8, 16, 32, 64, 128):
        for g in (cu - 9, cu - 8, cu - 1, cu, cu + 1, 2 * cu, 3 * cu + 7):
            out.update((g * gf - 1, g * gf, g * gf + 1))
    out.update((100000, 1 << 20, (1 << 31) - 1))
    return sorted(c for c in out if c >= 1)


def test_restated_rule_equals_the_librarys(pkg):
    fl = pkg.binding.debug_frames_launch
    checked = 0
    for n in [32] + launchref.SIZES + [16384]:
        for cu in CUS:
            counts = _threshold_counts(cu)
            for lut_len in (2, 256, 4096):           # 4096 = SP_MAX_LUT: beyond the byte tile's 256 colour indices, refused
                for count in counts:
                    got, want = fl(n, lut_len, count, cu), launchref.launch(n, lut_len, count, cu)
                    assert (got[:3] if got else None) == want, (n, cu, lut_len, count, got, want)
                    if got:
                        assert 0 < got[3] <= 160 * 1024
                        checked += 1
            # a batch launch: the groups are dealt already
            for gf in launchref.reachable_gf(n) if n in launchref.SIZES else [4]:
                for groups in (1, 7, 8, 9, cu - 1, cu, cu + 1, 3 * cu + 7):
                    got = fl(n, 256, groups, cu, gf)
                    assert (got[:3] if got else None) == launchref.launch(n, 256, groups, cu, gf), (n, cu, gf, groups)
    assert checked > 5000
    assert fl(64, 1, 100, 256) is None                # a one-entry LUT is the scratch kernel's
    with pytest.raises(pkg.SpectroplotError):
        fl(100, 256, 100, 256)                        # not a power of two
    with pytest.raises(pkg.SpectroplotError):
        fl(64, 256, 0, 256)


def test_plan_debug_launch_is_exported_and_checks_its_arguments(pkg):
    lib = C.CDLL(pkg.lib_path())
    assert hasattr(lib, "sp_plan_debug_launch") and hasattr(lib, "sp_debug_frames_launch")
    lib.sp_plan_debug_launch.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    used = C.c_size_t()
    assert lib.sp_plan_debug_launch(None, 1024, 4, None, None, 0, C.byref(used)) == -1


def test_cu_count_entries_check_their_arguments(pkg):
    """sp_context_debug_set_cu_count without a context; sp_debug_mean_launch (no device needed) against the grid the GPU tests expect:
    ceil(4 * cu / bands) pieces of the frames, ceil(frames / 32) at the most."""
    import test_cu_counts_gpu as gpu
    lib = C.CDLL(pkg.lib_path())
    lib.sp_context_debug_set_cu_count.argtypes = [C.c_void_p, C.c_int32]
    assert lib.sp_context_debug_set_cu_count(None, 0) == -1 and lib.sp_context_debug_set_cu_count(None, 8) == -1
    lib.sp_debug_mean_launch.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    out, used = (C.c_int64 * 3)(), C.c_size_t()
    assert lib.sp_debug_mean_launch(64, 300, 8, out, 3, C.byref(used)) == 0 and used.value == 3 and list(out) == [1, 10, 30]
    assert lib.sp_debug_mean_launch(64, 300, 8, out, 2, C.byref(used)) == -1 and used.value == 3      # capacity
    assert lib.sp_debug_mean_launch(64, 300, 8, None, 3, C.byref(used)) == -1 and lib.sp_debug_mean_launch(64, 300, 8, out, 3, None) == -1
    for bad in ((0, 300, 8), (64, 0, 8), (64, 300, 0)):
        assert lib.sp_debug_mean_launch(*bad, out, 3, C.byref(used)) == -1, bad
    for (cu, n, W), want in gpu.E_SHAPES.items():
        assert pkg.binding.debug_mean_launch(n, W, cu) == want == gpu._pieces(n, W, cu), (cu, n, W)
    for cu in (1, 8, 32, 256):
        for n in (1, 64, 65, 100, 1 << 20):
            for frames in (1, 31, 32, 33, 1000, 1 << 24):
                bands, pieces, per = pkg.binding.debug_mean_launch(n, frames, cu)
                assert (bands, pieces, per) == gpu._pieces(n, frames, cu) and (pieces - 1) * per < frames <= pieces * per


def test_reachable_gf_and_intervals():
    assert launchref.gf_pairs() == [(64, 128), (128, 64), (256, 32), (512, 16), (512, 32), (1024, 8), (1024, 16), (1024, 32), (2048, 4),
                                    (2048, 8), (2048, 16), (2048, 32), (4096, 4), (4096, 8), (4096, 16), (8192, 4), (8192, 8)]
    for cu in CUS:
        for n, gf in launchref.gf_pairs():
            lo, hi = launchref.frames_interval(n, gf, cu)
            assert launchref.batch_gf(n, lo, cu) == gf and (lo == 1 or launchref.batch_gf(n, lo - 1, cu) < gf)
            if hi is not None:
                assert launchref.batch_gf(n, hi, cu) == gf and launchref.batch_gf(n, hi + 1, cu) > gf
            else:
                assert launchref.batch_gf(n, 1 << 30, cu) == gf
    assert launchref.frames_interval(1024, 16, 256) == (8177, 16352) and launchref.frames_interval(1024, 32, 256) == (16353, None)
    assert [launchref.rounds(n, gf) for n, gf in ((64, 128), (512, 32), (1024, 8), (1024, 32), (2048, 4), (8192, 8))] == [1, 2, 1, 4, 1, 8]
    assert [launchref.halves(n, gf) for n, gf in launchref.gf_pairs()].count(True) == 1


def test_deal_covers_every_group_once():
    for cu in CUS:
        for groups in list(range(1, 50)) + [cu - 1, cu, cu + 1, 2 * cu - 1, 2 * cu, 2 * cu + 1, 3 * cu + 7, 5 * cu + 3]:
            grid = launchref.grid_for(groups, cu)
            assert grid % 8 == 0 and grid <= (cu + 7) // 8 * 8 and grid >= min(groups, cu)
            seen = []
            per_xcd, chunk = grid >> 3, (groups + 7) >> 3
            for b in range(grid):                     # the kernels' loop, spelled out (sp_frames_setup.inc.h, the group loop)
                g, mine = (b & 7) * chunk + (b >> 3), []
                while g < min(groups, ((b & 7) + 1) * chunk):
                    mine.append(g)
                    g += per_xcd
                seen += mine
                assert len(mine) == launchref.deal(groups, grid)[b]
            assert sorted(seen) == list(range(groups))
            assert launchref.deal_minmax(groups, grid) == (min(launchref.deal(groups, grid)), max(launchref.deal(groups, grid)))


@pytest.mark.parametrize("cu", CUS)
def test_chooser_reaches_every_shape_the_rule_allows(cu):
    unreachable = []
    for (n, gf), regime in itertools.product(launchref.gf_pairs(), launchref.REGIMES):
        got = {}
        for w4 in (False, True):
            ragged = not (gf == 4 and w4)             # 4-frame groups: a width that is a multiple of 4 has no ragged last group
            W = got[w4] = launchref.choose_width(n, cu, gf, regime, w4, ragged)
            if W is None:
                continue
            g, groups, grid = launchref.launch(n, 256, W, cu)
            assert g == gf and groups % 8 != 0 and (W % 4 == 0) == w4 and (W % gf != 0) == ragged, (n, gf, regime, W)
            assert launchref.regime_of(groups, grid) == regime
            lo, hi = launchref.deal_minmax(groups, grid)
            assert {"one": hi == 1 and groups < grid, "mixed": (lo, hi) == (1, 2), "many": lo >= 3}[regime], (n, gf, regime, W, lo, hi)
        assert (got[False] is None) == (got[True] is None), (n, gf, regime, got)
        if got[False] is None:
            unreachable.append((n, gf, regime))
    assert sorted(unreachable) == launchref.unreachable_by_rule(cu)
    # 9 pairs above the smallest gf: `one`, and `mixed` where the grid is the CU count; 9 pairs below the largest: `many` on 8 and 20 CUs
    assert len(unreachable) == {8: 27, 20: 18}.get(cu, 18)
    assert sum(r == "many" for _, _, r in unreachable) == (9 if cu in SHORT else 0)
    assert sum(r == "mixed" for _, _, r in unreachable) == (9 if cu % 8 == 0 else 0)


def test_what_the_lattice_covers():
    fr = launchref.frames_lattice()
    pairs = launchref.gf_pairs()
    plain = [c for c in fr if not c["oob"]]
    assert len({launchref.case_id(c) for c in fr}) == len(fr)
    assert {(c["n"], c["gf"], c["loader"]) for c in plain} == {(n, gf, l) for n, gf in pairs for l in launchref.LOADERS}
    assert {(c["n"], c["loader"], c["ch"]) for c in plain} == {(n, l, ch) for n in launchref.SIZES for l in launchref.LOADERS for ch in (False, True)}
    for n, gf in pairs:
        here = [c for c in plain if (c["n"], c["gf"]) == (n, gf)]
        assert {c["wf"] for c in here} == {False, True} and {c["fast"] for c in here} == {False, True}
        assert {c["slow_by"] for c in here} == {None, "width", "pointer"}
        assert {c["regime"] for c in here} == set(launchref.REGIMES if gf == launchref.reachable_gf(n)[0] else ["many"])
        assert len({c["stride"] for c in here}) == 3
    hv = [c for c in plain if launchref.halves(c["n"], c["gf"])]
    assert {c["loader"] for c in hv} == set(launchref.LOADERS) and any(c["ch"] for c in hv) and any(c["wf"] for c in hv)
    assert sum(c["oob"] for c in fr) == 2 and all(c["regime"] == "many" and c["loader"] == 0 for c in fr if c["oob"])
    for cu in CUS:
        if cu not in SHORT:
            assert not {(c["n"], c["gf"], c["regime"]) for c in fr} & set(launchref.unreachable_by_rule(cu))

    pk = launchref.peak_lattice()
    assert len({launchref.case_id(c) for c in pk}) == len(pk) == 30
    for n in launchref.PEAK_SIZES:
        here = [c for c in pk if c["n"] == n]
        assert {c["loader"] for c in here} == set(launchref.LOADERS)
        assert {c["ch"] for c in here} == {c["wf"] for c in here} == {c["fast"] for c in here} == {False, True}
        assert {c["M"] for c in here} == {2, 3}
        gfs = launchref.reachable_gf(n)
        assert {(c["gf"], c["regime"]) for c in here} == {(gfs[0], "mixed"), (gfs[0], "many")} | {(g, "many") for g in gfs[1:]}
    assert any(launchref.halves(c["n"], c["gf"]) for c in pk)

    for cu in CUS:
        assert len(launchref.reachable(pk, cu)) == (25 if cu in SHORT else 30)

    bt = launchref.batch_lattice()
    assert [(c["n"], c["gf"]) for c in bt] == launchref.gf_pairs(launchref.BATCH_SIZES)
    for cu in CUS:
        for c in bt:
            w = launchref.batch_widths(c["n"], c["gf"], cu)
            gf = c["gf"]
            assert w[:5] == [1, gf - 1, gf, gf + 1, 0] and all(x % gf for x in w[5:]) and launchref.batch_gf(c["n"], sum(w), cu) == gf


def test_cells_out_of_reach_at_the_counts_the_gpu_runs():
    """What tests/test_cu_counts_gpu.py may leave out, and no more: of the 122 k_frames cases every one has a width at 16, 24, 32, 64, 104
    and 128 CUs; at 8 and at 20 the 34 `many` cases of every gf below the largest have none (their cells are unreachable_by_rule's), and
    every other case has one.  Of the 30 peak cases 5 are out of reach there.  The thinned lattice keeps one case per (n, gf) within reach."""
    import test_cu_counts_gpu as gpu
    fr, pk = launchref.frames_lattice(), launchref.peak_lattice()
    assert len(fr) == 122 and len(pk) == 30
    assert set(gpu.FRAMES_CUS) | set(gpu.THIN_CUS) == {8, 16, 20, 24, 32, 128} and set(gpu.LATTICE_CUS) == {16, 8}
    for cu in (8, 16, 20, 24, 32, 64, 104, 128):
        got = {"frames": [], "peak": []}
        for name, cases in (("frames", fr), ("peak", pk)):
            for c in cases:
                w4 = c["fast"] or c["slow_by"] == "pointer"
                if launchref.choose_width(c["n"], cu, c["gf"], c["regime"], w4, ragged_group=not (c["gf"] == 4 and w4)) is None:
                    got[name].append(launchref.case_id(c))
            keep = {launchref.case_id(c) for c in launchref.reachable(cases, cu)}
            assert set(got[name]) == {launchref.case_id(c) for c in cases} - keep, (cu, name)
        assert (len(got["frames"]), len(got["peak"])) == ((34, 5) if cu in SHORT else (0, 0)), cu
        if cu == 8:
            got8 = got
        if cu in SHORT:
            left = [c for c in fr if launchref.case_id(c) in got["frames"]]
            assert all(c["regime"] == "many" and c["gf"] != launchref.reachable_gf(c["n"])[-1] for c in left)
            assert {(c["n"], c["gf"]) for c in left} == {(n, gf) for n in launchref.SIZES for gf in launchref.reachable_gf(n)[:-1]}
    # the full lattices run at 16, 32 and 8 CUs (peak: 16 and 8): 8 is the one count at which the GPU module leaves cells out
    assert gpu.SKIPPED == {("frames", 8): sorted(got8["frames"]), ("peak", 8): sorted(got8["peak"])}
    for cu in gpu.THIN_CUS:
        thin = gpu.thinned(cu)
        assert {(c["n"], c["gf"]) for c in thin} == set(launchref.gf_pairs()) and len(thin) == 17
        assert {c["loader"] for c in thin} == set(launchref.LOADERS) and {c["ch"] for c in thin} == {c["wf"] for c in thin} == {False, True}
        assert {c["fast"] for c in thin} == {False, True} and thin == launchref.reachable(thin, cu)
    # parts B and C: every case has a width at both counts, and the rotations reach every loader, write-out and layout
    for cu in gpu.LATTICE_CUS:
        for c in launchref.batch_lattice():
            assert launchref.batch_gf(c["n"], sum(launchref.batch_widths(c["n"], c["gf"], cu)), cu) == c["gf"]
        for c in gpu.index_cases():
            W = gpu.indexref.choose_width(c["n"], cu, c["gf"], c["regime"], c["writeout"])
            assert W and launchref.launch(c["n"], 256, W, cu)[0] == c["gf"] and gpu.indexref.built(c["n"], c["loader"], c["ch"])
        for c in gpu.plane_cases(("one", "mixed", "many")):
            W = launchref.choose_width(c["n"], cu, c["gf"], c["regime"], w4=False)
            g, groups, grid = launchref.launch(c["n"], 256, W, cu)
            assert g == c["gf"] and W % g != 0 and groups % 8 != 0 and launchref.regime_of(groups, grid) == c["regime"]
    ix = gpu.index_cases()
    assert len(ix) == 2 * len(launchref.SIZES) and {c["loader"] for c in ix} == set(launchref.LOADERS)
    assert {c["writeout"] for c in ix} == {"fast", "w4", "w1", "p1", "p4"} and {c["ch"] for c in ix} == {c["wf"] for c in ix} == {False, True}
    assert any(launchref.halves(c["n"], c["gf"]) for c in ix)
    assert len(gpu.expected_ids()) == 568
