"""Every launch-shape rule that reads the CU count, on the GPU at CU counts other than the part's own.

sp_context_debug_set_cu_count (Context.set_cu_count) replaces the count a context's launches are shaped by; this module runs the
kernels at 1, 8, 16, 20, 24, 32 and 128 CUs on a context of its own, every override inside try / finally ending in set_cu_count(0).
At 16 CUs a workgroup of a full grid strides over its XCD's groups by 2 (per_xcd = gridDim.x >> 3), at 8 by 1, at 20 and 24 by 3 - at
20 the grid, rounded up to the 8 XCDs, exceeds the CU count - at 32 by 4, at 128 by 16; the part's own 256 gives 32, the only stride
every other module runs.  Every case is ONE launch whose shape is confirmed through the library's debug entries at the overridden count
before anything is rendered, and whose whole reply is compared bit for bit, no tolerance, with the reference its kernel's own module
uses.  Helpers - captures, guards, garbage fills, comparisons, the look-ahead pool of references - are those of
tests/test_launch_shapes_gpu.py, test_index_launch_shapes_gpu.py and test_scratch_shapes_gpu.py.

A  k_frames: launchref.frames_lattice() whole at 16 and 32 CUs, its cells within reach at 8 (launchref.reachable), and thinned() -
   one case per (n, gf) - at 20, 24 and 128.
B  k_frames_peak and k_frames_batch: peak_lattice() (the cells within reach) and batch_lattice() at 16 and 8 CUs.
C  k_frames_index, k_frames_traces, k_frames_power: the regimes of their modules' launch-shape tests at 16 and 8 CUs, every n.
D  the scratch kernels at 8 CUs: 32 workgroups, 100 frames - three or four columns per workgroup.
E  k_mean_accumulate at 1 and 8 CUs (pieces of unequal length, ceil(frames / 32) pieces on either side of the part's bound) and
   k_power_to_db at 1 CU (four trips of the grid-stride loop, the last ragged).
F  one request of every reply kind at 1, 8, 20, 32 CUs and the part's own: every reply equal to the reference and to the first.
The last test asserts that every case ran, apart from the cells tests/test_launch_shapes_cpu.py pins as out of reach (SKIPPED)."""
import contextlib
import functools
import time

import numpy as np
import pytest

import bandref
import blockmeanref
import burstref
import densityref
import indexref
import launchref
import meanref
import momentref
import occref
import peakref
import powerref
import pulseref
import quantileref
import scratchref
import siggen
import test_index_launch_shapes_gpu as shapes
import test_launch_shapes_gpu as base
import test_scratch_shapes_gpu as ss
import tracesref
import trackref
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GAIN, RANGE = base.GAIN, base.RANGE
FRAMES_CUS = (16, 32, 8)            # A: the whole lattice (what is within reach of it)
THIN_CUS = (20, 24, 128)            # A: one case per (n, gf)
LATTICE_CUS = (16, 8)               # B, C
SCRATCH_CU = 8                      # D
FRAME_SIZES = [64, 128, 256, 512, 1024]     # k_frames_traces, k_frames_power

FRAMES, PEAK, BATCH = launchref.frames_lattice(), launchref.peak_lattice(), launchref.batch_lattice()
# what the module leaves out: the cells no width reaches (tests/test_launch_shapes_cpu.py pins this list against the chooser)
SKIPPED = {(name, cu): sorted(launchref.case_id(c) for c in cases if c not in launchref.reachable(cases, cu))
           for name, cases in (("frames", FRAMES), ("peak", PEAK)) for cu in (8,)}
RAN = set()
TIMES = {}

pkg = base.pkg


@pytest.fixture(scope="module")
def ctx(pkg):
    """The module's own context: no other module sees an override."""
    c = pkg.Context(0)
    yield c
    c.set_cu_count(0)
    c.close()


@pytest.fixture(scope="module")
def own(ctx):
    """The part's own CU count."""
    ctx.set_cu_count(0)
    return _reported(ctx)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


def _reported(ctx):
    """The CU count sp_plan_debug_launch reports on this context."""
    win, weight = pyoracle.window("hann", 64)
    plan = ctx.plan("CU8", 64, win, 1.0 / weight, GAIN, RANGE, base._lut())
    try:
        return plan.debug_launch(2 * 64 * 4, 4)["cu_count"]
    finally:
        plan.close()


@contextlib.contextmanager
def at(ctx, cu):
    """The context's launches shaped for `cu` CUs within the block, for the part's own count behind it."""
    ctx.set_cu_count(cu)
    try:
        yield
    finally:
        ctx.set_cu_count(0)


def _per_xcd(d, cu):
    """A launch with as many groups as CUs or more has the full grid: its workgroups stride by grid_for(cu, cu) / 8."""
    if d["groups"] >= cu:
        assert d["grid"] == launchref.grid_for(cu, cu) and d["grid"] >> 3 == {8: 1, 16: 2, 20: 3, 24: 3, 32: 4, 128: 16}[cu], d


# ---------------------------------------------------------------------------------------------------------------------- A: k_frames
def thinned(cu):
    """One k_frames case per (n, gf) within reach on a cu-CU part: the largest regime in reach above the smallest gf (`many`; `mixed` where
    the rule puts `many` out of reach), the three regimes in turn at the smallest; loader, L/R split, layout, write-out and stride rotate."""
    out_of_reach = set(launchref.unreachable_by_rule(cu))
    cases = []
    for k, (n, gf) in enumerate(launchref.gf_pairs()):
        order = [launchref.REGIMES[(k + j) % 3] for j in range(3)] if gf == launchref.reachable_gf(n)[0] else ["many", "mixed", "one"]
        regime = [r for r in order if (n, gf, r) not in out_of_reach][0]
        loader, fast = launchref.LOADERS[k % 6], k % 3 != 2
        cases.append(dict(n=n, gf=gf, regime=regime, loader=loader, fmt=launchref.LOADER_FORMATS[loader][(k // 6) % 2], ch=k % 2 == 1,
                          wf=(k // 2) % 2 == 1, fast=fast, slow_by=None if fast else ("width", "pointer")[(k // 3) % 2],
                          stride=launchref.STRIDES[k % 3], oob=False))
    return cases


A_CASES = [(cu, c) for cu in FRAMES_CUS for c in launchref.reachable(FRAMES, cu)] + [(cu, c) for cu in THIN_CUS for c in thinned(cu)]


def _id(kind, cu, c):
    return "%s_cu%d_%s" % (kind, cu, c if isinstance(c, str) else launchref.case_id(c))


@pytest.fixture(scope="module")
def frames_ahead():
    pyoracle.lib()

    def make(item):
        cu, c = item
        n, W = c["n"], base._width(c, cu)
        data = base._capture(c["fmt"], n, W, c["gf"], c["stride"], c["oob"])
        win, weight = pyoracle.window("blackmanHarris" if c["wf"] else "hann", n)
        want = pyoracle.render(c["fmt"], data, n, win, 1.0 / weight, GAIN, RANGE, base._lut(), W, c["ch"], c["wf"])
        return W, data, win, weight, want

    a = base._Ahead(A_CASES, make)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("k", range(len(A_CASES)), ids=[_id("frames", cu, c) for cu, c in A_CASES])
def test_k_frames_whole_reply(pkg, ctx, frames_ahead, k):
    cu, c = A_CASES[k]
    what = _id("frames", cu, c)
    W, data, win, weight, want = frames_ahead.get(k)
    lut = base._lut()
    expect = base._expect_launch(c, cu, "frames", W)

    def check(d):
        expect(d)
        _per_xcd(d, cu)

    plan = ctx.plan(c["fmt"], c["n"], win, 1.0 / weight, GAIN, RANGE, lut, c["ch"], c["wf"])
    try:
        with at(ctx, cu):
            got = base._run(ctx, plan, data, W, c["n"], len(lut), c["slow_by"] == "pointer", check, what)
    finally:
        plan.close()
    base._same(got, want, "%s W=%d" % (what, W))
    RAN.add(what)


# ------------------------------------------------------------------------------------------------ B: k_frames_peak, k_frames_batch
B_PEAK = [(cu, c) for cu in LATTICE_CUS for c in launchref.reachable(PEAK, cu)]
B_BATCH = [(cu, k) for cu in LATTICE_CUS for k in range(len(BATCH))]


@pytest.fixture(scope="module")
def peak_ahead():
    pyoracle.lib()

    def make(item):
        cu, c = item
        n, W, M = c["n"], base._width(c, cu), c["M"]
        sw = siggen.SAMPLE_WIDTH[c["fmt"]]
        samples = n + (W - 1) * M * n + (W - 1) // 2 + 1          # a fractional stride: the last column has one sub-frame only
        data = base._trinoise(c["fmt"], samples)
        base._silence(data, sw, samples, n, W, c["gf"])
        win, weight = pyoracle.window("hann", n)
        want = peakref.expected(c["fmt"], data, n, win, 1.0 / weight, GAIN, RANGE, base._lut(), W, c["ch"], c["wf"])
        assert want["M"] == M and want["counts"][-1] < M and all(v == M for v in want["counts"][:-1])
        return W, data, win, weight, {k: v for k, v in want.items() if k not in ("jstar", "counts")}

    a = base._Ahead(B_PEAK, make, depth=4)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("k", range(len(B_PEAK)), ids=[_id("peak", cu, c) for cu, c in B_PEAK])
def test_k_frames_peak_whole_reply(pkg, ctx, peak_ahead, k):
    cu, c = B_PEAK[k]
    what = _id("peak", cu, c)
    W, data, win, weight, want = peak_ahead.get(k)
    lut = base._lut()
    expect = base._expect_launch(c, cu, "frames_peak", W, c["M"])

    def check(d):
        expect(d)
        _per_xcd(d, cu)

    plan = ctx.plan(c["fmt"], c["n"], win, 1.0 / weight, GAIN, RANGE, lut, c["ch"], c["wf"], detector="peak")
    try:
        with at(ctx, cu):
            got = base._run(ctx, plan, data, W, c["n"], len(lut), c["slow_by"] == "pointer", check, what)
    finally:
        plan.close()
    base._same(got, want, "%s W=%d" % (what, W))
    RAN.add(what)


@pytest.mark.parametrize("item", B_BATCH, ids=[_id("batch", cu, BATCH[k]) for cu, k in B_BATCH])
def test_k_frames_batch_whole_replies(pkg, ctx, item):
    """tests/test_launch_shapes_gpu.py's batch case with launchref.batch_widths(n, gf, cu) for the overridden count: its work list
    through sp_debug_batch_plan at that count, one sp_plan_execute_batch, every item against the oracle."""
    cu, k = item
    mine = set(base.RAN["batch"])           # (that module's record of what it ran itself stays its own)
    try:
        with at(ctx, cu):
            assert _reported(ctx) == cu
            base.test_k_frames_batch_whole_replies(pkg, ctx, cu, k)
    finally:
        base.RAN["batch"] = mine
    RAN.add(_id("batch", cu, BATCH[k]))


# ------------------------------------------------------------------------------- C: k_frames_index, k_frames_traces, k_frames_power
def _cells(n, regimes):
    """(gf, regime) as the kernels' own launch-shape tests take them: the smallest gf below `many`, the largest at `many`."""
    gfs = launchref.reachable_gf(n)
    return [(gfs[-1] if r == "many" else gfs[0], r) for r in regimes]


def index_cases():
    """k_frames_index at every n in `mixed` and `many`; loader, L/R split, layout and write-out rotate.  (The write-out's width property
    is the first of the rotation that a width of the cell has on both CU counts: few group counts are `mixed` on 8 CUs.)"""
    cases = []
    for ni, n in enumerate(launchref.SIZES):
        for j, (gf, regime) in enumerate(_cells(n, ("mixed", "many"))):
            i = (ni + 3 * j) % 6
            loader = launchref.LOADERS[i]
            turn = [indexref.WRITEOUTS[(ni + 2 * j + t) % 6] for t in range(6)]
            writeout = [w for w in turn if all(indexref.choose_width(n, cu, gf, regime, w) for cu in LATTICE_CUS)][0]
            cases.append(dict(n=n, gf=gf, regime=regime, loader=loader, fmt=launchref.LOADER_FORMATS[loader][(ni + j) % 2],
                              ch=(ni + j) % 2 == 1 and indexref.built(n, loader, True), wf=(ni // 2 + j) % 2 == 1, writeout=writeout))
    return cases


def plane_cases(regimes):
    """k_frames_traces / k_frames_power at every n they take; formats and the L/R split rotate as in their modules."""
    fmts = ["CS16", "CU8", "CF32", "CS12", "CU4"]
    return [dict(n=n, gf=gf, regime=regime, fmt=fmts[(k + j) % 5], ch=(k + j) % 2 == 1)
            for k, n in enumerate(FRAME_SIZES) for j, (gf, regime) in enumerate(_cells(n, regimes))]


C_INDEX = [(cu, c) for cu in LATTICE_CUS for c in index_cases()]
C_TRACES = [(cu, c) for cu in LATTICE_CUS for c in plane_cases(("mixed", "many"))]
C_POWER = [(cu, c) for cu in LATTICE_CUS for c in plane_cases(("one", "mixed", "many"))]


def _plane_id(c):
    return "n%d_gf%d_%s_%s%s" % (c["n"], c["gf"], c["regime"], c["fmt"], "_lr" if c["ch"] else "")


@pytest.fixture(scope="module")
def index_ahead():
    pyoracle.lib()

    def make(item):
        cu, c = item
        n = c["n"]
        W = indexref.choose_width(n, cu, c["gf"], c["regime"], c["writeout"])
        data = base._capture(c["fmt"], n, W, c["gf"], "overlap")
        win, weight = pyoracle.window("blackmanHarris" if c["wf"] else "hann", n)
        want = pyoracle.render(c["fmt"], data, n, win, 1.0 / weight, GAIN, RANGE, base._lut(), W, c["ch"], c["wf"])
        return W, data, win, weight, want

    a = base._Ahead(C_INDEX, make)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("k", range(len(C_INDEX)), ids=[_id("index", cu, indexref.case_id(c)) for cu, c in C_INDEX])
def test_k_frames_index_whole_reply(pkg, ctx, index_ahead, k):
    cu, c = C_INDEX[k]
    what = _id("index", cu, indexref.case_id(c))
    n = c["n"]
    W, data, win, weight, want = index_ahead.get(k)
    lut = base._lut()

    def check(d):
        assert d["kernel"] == "frames_index" and d["cu_count"] == cu and d["log2n"] == n.bit_length() - 1, d
        assert d["gf"] == c["gf"] and d["groups"] == -(-W // c["gf"]) and d["grid"] == launchref.grid_for(d["groups"], cu), d
        assert launchref.regime_of(d["groups"], d["grid"]) == c["regime"] and d["groups"] % 8 != 0, d
        assert d["prefetch"] == c["loader"] and d["rgba_fast"] == int(c["writeout"] == "fast") and d["channel_mode"] == int(c["ch"]), d
        _per_xcd(d, cu)

    plan = ctx.plan(c["fmt"], n, win, 1.0 / weight, GAIN, RANGE, lut, c["ch"], c["wf"])
    try:
        with at(ctx, cu):
            assert plan.index_kernel_name_for(data.size, W) == "frames_index"
            got = shapes.run(ctx, plan, data, W, n, len(lut), indexref.misalign(c["writeout"]), check, what)
    finally:
        plan.close()
    shapes.same(got, want, "%s W=%d" % (what, W))
    RAN.add(what)


@functools.lru_cache(maxsize=None)
def _plane_request(cu, n, gf, regime, fmt, ch):
    """(W, capture, taper, block_norm) of a traces / power case: a ragged last group, a group count that is no multiple of 8, a
    fractional stride of about 67 samples."""
    W = launchref.choose_width(n, cu, gf, regime, w4=False)
    assert W is not None and W % gf != 0
    data = siggen.generate(fmt, base.GEN, n + (W - 1) * 67 + 29)
    win, weight = pyoracle.window("hann", n)
    return W, data, win, 1.0 / weight


def _confirm_plane_launch(pkg, plan, c, cu, W, nbytes):
    """k_frames_traces and k_frames_power launch by the rule k_frames launches by: the plan's own answer at the overridden count."""
    d = plan.debug_launch(nbytes, W)
    assert d["kernel"] == "frames" and d["cu_count"] == cu, d
    assert (d["gf"], d["groups"], d["grid"]) == launchref.launch(c["n"], 256, W, cu), d
    assert pkg.binding.debug_frames_launch(c["n"], 256, W, cu)[:3] == (d["gf"], d["groups"], d["grid"])
    assert d["gf"] == c["gf"] and d["groups"] % 8 != 0 and launchref.regime_of(d["groups"], d["grid"]) == c["regime"], d
    assert launchref.halves(c["n"], c["gf"]) == (c["n"] == 1024 and c["regime"] == "many")
    _per_xcd(d, cu)


@pytest.mark.parametrize("item", C_TRACES, ids=[_id("traces", cu, _plane_id(c)) for cu, c in C_TRACES])
def test_k_frames_traces_whole_reply(pkg, ctx, item):
    cu, c = item
    what = _id("traces", cu, _plane_id(c))
    n = c["n"]
    W, data, win, bn = _plane_request(cu, n, c["gf"], c["regime"], c["fmt"], c["ch"])
    want = tracesref.expected(c["fmt"], data, n, win, bn, GAIN, RANGE, W, c["ch"])
    assert len(np.unique(want["trace_min"])) >= n // 2 and len(np.unique(want["trace_max"])) >= n // 2
    plan = ctx.plan(c["fmt"], n, win, bn, GAIN, RANGE, base._lut(), c["ch"])
    d_in, lo, hi = ctx.alloc(data.size + 16), ss._Dev(ctx, 8 * n), ss._Dev(ctx, 8 * n)
    try:
        ctx.upload(d_in, data)
        with at(ctx, cu):
            _confirm_plane_launch(pkg, plan, c, cu, W, data.size)
            assert plan.traces_kernel_name_for(data.size, W) == "frames_traces"
            plan.execute_traces(d_in, data.size, W, lo.ptr, hi.ptr)
            ctx.synchronize()
        got = {"trace_min": lo.read(np.float64, what), "trace_max": hi.read(np.float64, what)}
    finally:
        lo.free()
        hi.free()
        ctx.free(d_in)
        plan.close()
    tracesref.assert_same(got, want, "%s W=%d" % (what, W))
    RAN.add(what)


@pytest.mark.parametrize("item", C_POWER, ids=[_id("power", cu, _plane_id(c)) for cu, c in C_POWER])
def test_k_frames_power_whole_reply(pkg, ctx, item):
    cu, c = item
    what = _id("power", cu, _plane_id(c))
    n = c["n"]
    W, data, win, bn = _plane_request(cu, n, c["gf"], c["regime"], c["fmt"], c["ch"])
    want = powerref.expected(c["fmt"], data, n, win, bn, GAIN, RANGE, W, c["ch"])["power"]
    powerref.assert_telling(want[:, 1:] if c["ch"] else want, what)          # (row 0 of an L/R split is bin n / 2: zero)
    plan = ctx.plan(c["fmt"], n, win, bn, GAIN, RANGE, base._lut(), c["ch"])
    d_in, pl = ctx.alloc(data.size + 16), ss._Dev(ctx, 8 * W * n)
    try:
        ctx.upload(d_in, data)
        with at(ctx, cu):
            _confirm_plane_launch(pkg, plan, c, cu, W, data.size)
            assert plan.power_kernel_name_for(data.size, W) == "frames_power"
            plan.execute_power(d_in, data.size, W, pl.ptr)
            ctx.synchronize()
        got = pl.read(np.float64, what).reshape(W, n)
    finally:
        pl.free()
        ctx.free(d_in)
        plan.close()
    powerref.assert_same(got, want, "%s W=%d" % (what, W))
    RAN.add(what)


# --------------------------------------------------------------------------------------------------------- D: the scratch kernels
D_WIDTH = 100
D_CASES = [ss._case("D", kind, n, ("CS16", "CU8", "CF32", "CS12")[(i + j) % 4], ch=(i + j) % 2 == 1, wf=kind in ("image", "peak") and (i + j // 2) % 2 == 0,
                    plus=D_WIDTH, hop=n // 8 + 3, M=2 if kind == "peak" else 1, force=n in (2048, 8192))
           for i, n in enumerate((32, 2048, 8192, 16384)) for j, kind in enumerate(("image", "peak", "traces", "power"))]


@pytest.fixture(scope="module")
def scratch_ahead():
    pyoracle.lib()
    a = base._Ahead(D_CASES, lambda c: ss._make(c, SCRATCH_CU), depth=3)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("k", range(len(D_CASES)), ids=[_id("scratch", SCRATCH_CU, c["id"]) for c in D_CASES])
def test_scratch_whole_reply(pkg, ctx, scratch_ahead, k):
    """32 workgroups, the part's bound at 8 CUs, serve 100 columns: four each for the first four, three for the others."""
    c, cu = D_CASES[k], SCRATCH_CU
    made = scratch_ahead.get(k)
    W, B = made[:2]
    slabs = scratchref.SLABS[c["kind"]]
    assert (W, B) == (D_WIDTH, 4 * cu) and pkg.binding.debug_scratch_launch(c["n"], slabs, W, cu) == (4 * cu, c["n"] >= 4096)
    assert {len(scratchref.columns_of(b, W, B)) for b in range(B)} == {3, 4}
    assert B < scratchref.CAP_BYTES // (8 * slabs * c["n"]) and B < W         # neither the cap nor the frames are the bound
    with at(ctx, cu):
        ss.run_case(pkg, ctx, cu, c, made)
    RAN.add(_id("scratch", cu, c["id"]))


# ------------------------------------------------------------------------------------------- E: k_mean_accumulate, k_power_to_db
E_MEAN = [(cu, n, W) for cu in (1, 8) for n in (64, 100) for W in (33, 300, 2049)]


# (bands of 64 rows, pieces, frames per piece) of k_mean_accumulate's grid: ceil(4 * cu / bands) pieces, ceil(frames / 32) at the most
E_SHAPES = {(1, 64, 33): (1, 2, 17), (1, 64, 300): (1, 4, 75), (1, 64, 2049): (1, 4, 513),
            (1, 100, 33): (2, 2, 17), (1, 100, 300): (2, 2, 150), (1, 100, 2049): (2, 2, 1025),
            (8, 64, 33): (1, 2, 17), (8, 64, 300): (1, 10, 30), (8, 64, 2049): (1, 32, 65),
            (8, 100, 33): (2, 2, 17), (8, 100, 300): (2, 10, 30), (8, 100, 2049): (2, 16, 129)}


def _pieces(n, frames, cu):
    """mean_pieces and the frames per piece restated: about four workgroups per CU over the bands of 64 rows, no piece below 32 frames."""
    bands = -(-n // 64)
    pieces = max(1, min(-(-4 * cu // bands), -(-frames // 32)))
    return bands, pieces, -(-frames // pieces)


@functools.lru_cache(maxsize=None)
def _planted(n, W):
    plane = meanref.synthetic_plane(1000 * n + W, W, n)
    plane.setflags(write=False)
    return plane, meanref.expected(plane)


@pytest.mark.parametrize("item", E_MEAN, ids=["mean_cu%d_n%d_W%d" % t for t in E_MEAN])
def test_power_mean_of_planted_planes(pkg, ctx, item):
    from test_mean_gpu import _power_mean
    cu, n, W = item
    what = "mean_cu%d_n%d_W%d" % item
    plane, want = _planted(n, W)
    shape = pkg.binding.debug_mean_launch(n, W, cu)
    assert shape == _pieces(n, W, cu) == E_SHAPES[item], (what, shape)
    bands, pieces, per = shape
    assert (pieces - 1) * per < W <= pieces * per                         # every piece holds frames; the last is the short one
    if W != 300:
        assert W % per != 0, (what, shape)                                # pieces of unequal length
    with at(ctx, cu):
        assert _reported(ctx) == cu
        got = _power_mean(ctx, plane, what)
    meanref.assert_same(got, want, what)
    RAN.add(what)


E_DB = [(16 * 256 * 3 + 5, "in"), (16 * 256 * 3 + 5, "out"), (16 * 256 - 1, "in"), (16 * 256 - 1, "out")]


@pytest.mark.parametrize("count,place", E_DB, ids=["db_cu1_%d_%s" % t for t in E_DB])
def test_power_to_db_at_one_cu(ctx, count, place):
    """16 workgroups of 256 threads at 1 CU: 16 * 256 * 3 + 5 elements take four trips of the grid-stride loop, the last of 5 elements;
    16 * 256 - 1 take one by 16 workgroups, the last one ragged (at the part's own count: 49 workgroups and one trip)."""
    what = "db_cu1_%d_%s" % (count, place)
    step = 16 * 1 * 256
    assert -(-count // step) == (4 if count > step else 1) and count % 256 != 0
    rng = np.random.default_rng(count)
    values = rng.random(count) * np.exp2(rng.integers(-60, 40, count))
    values[::97] = 0.0                                                           # (log10(0) = -inf)
    n = 64
    win, weight = pyoracle.window("hann", n)
    want = meanref.db_of(values, 1.0 / weight, GAIN)
    plan = ctx.plan("CS16", n, win, 1.0 / weight, GAIN, RANGE, base._lut())
    src, dst = ss._Dev(ctx, 8 * count), ss._Dev(ctx, 8 * count)
    try:
        ctx.upload(src.ptr, values.view(np.uint8))
        with at(ctx, 1):
            assert plan.debug_launch(2 * n * 4, 4)["cu_count"] == 1
            plan.power_to_db(src.ptr, count, src.ptr if place == "in" else dst.ptr)
            ctx.synchronize()
        got = (src if place == "in" else dst).read(np.float64, what)
        if place == "out":
            assert np.array_equal(src.read(np.float64, what).view(np.uint64), values.view(np.uint64)), what + ": the source changed"
        else:
            assert (dst.read(np.uint8, what) == 0xAB).all(), what + ": the other plane was written"
    finally:
        src.free()
        dst.free()
        plan.close()
    meanref.assert_same(got, want, what)
    RAN.add(what)


# ------------------------------------------------------------------------------------------------------------------- F: invariance
F_N, F_W, F_FMT, F_M = 256, 300, "CS16", 4
F_CUS = (1, 8, 20, 32, 0)                    # 0: the part's own
F_KINDS = ("image", "peak", "traces", "index", "density", "power", "mean", "blockmean", "bandpower", "moments", "track", "occupancy", "quantile",
           "bursts", "pulses", "batch")
F_GROUPS = (12, 7)                           # block means: a group that divides the width and one that leaves a last column of 6 frames
F_ORDER = 2                                  # moments 0, 1, 2 on the standard bands
F_BATCH = (1, 31, 0, 77, 300)
FIRST = {}


@functools.lru_cache(maxsize=None)
def _f_request():
    """The capture every kind renders (the peak plan: one of three sub-frames per column), the batch's captures, and every reference."""
    n, W, lut = F_N, F_W, base._lut()
    assert W % F_GROUPS[0] == 0 and W % F_GROUPS[1] == 6
    win, weight = pyoracle.window("hann", n)
    bn = 1.0 / weight
    data = base._trinoise(F_FMT, n + (W - 1) * (n // 2 + 3) + 1, seed=6)
    peak_data = base._trinoise(F_FMT, n + (W - 1) * 3 * n + (W - 1) // 2 + 1, seed=7)
    items = [base._trinoise(F_FMT, 3 * n if w == 0 else n + (w - 1) * (n // 4) + (w - 1) // 3 + 1, seed=8 + j) for j, w in enumerate(F_BATCH)]
    image = pyoracle.render(F_FMT, data, n, win, bn, GAIN, RANGE, lut, W)
    plane = powerref.expected(F_FMT, data, n, win, bn, GAIN, RANGE, W)["power"]
    powerref.assert_telling(plane, "F")
    bands = bandref.standard_bands(n)
    sums = bandref.expected(plane, bands)
    median = np.sort(sums, axis=1)[:, (W - 1) // 2]
    hi, lo = 4.0 * median, 2.0 * median
    thr = occref.planted_thresholds(plane)
    ranks = quantileref.standard_ranks(W)
    peak = peakref.expected(F_FMT, peak_data, n, win, bn, GAIN, RANGE, lut, W)
    assert peak["M"] == 3
    want = {"image": image, "peak": {k: v for k, v in peak.items() if k not in ("jstar", "counts", "M")}, "index": image,
            "traces": tracesref.expected(F_FMT, data, n, win, bn, GAIN, RANGE, W), "density": densityref.expected(image, n, len(lut), W, False),
            "power": plane, "mean": meanref.expected(plane), "blockmean": [blockmeanref.expected(plane, g) for g in F_GROUPS],
            "bandpower": sums, "moments": momentref.expected(plane, bands, F_ORDER), "track": trackref.expected(plane, bands),
            "occupancy": occref.expected(plane, thr, bands), "quantile": quantileref.expected(plane, ranks),
            "bursts": burstref.expected(sums, hi, lo, F_M), "pulses": pulseref.expected(sums, hi, lo, F_M),
            "batch": [pyoracle.render(F_FMT, d, n, win, bn, GAIN, RANGE, lut, w) for d, w in zip(items, F_BATCH)]}
    return dict(win=win, bn=bn, data=data, peak_data=peak_data, items=items, bands=bands, hi=hi, lo=lo, thr=thr, ranks=ranks, want=want)


def _f_replies(ctx, cu, what):
    """Every kind's reply to the request on this context as it stands, each checked against its reference; -> {kind: arrays} for the
    comparison with the first count's."""
    from test_band_gpu import _execute_bandpower
    from test_blockmean_gpu import _execute_blockmean
    from test_mean_gpu import _execute_mean
    from test_moments_gpu import _execute_moments
    from test_occupancy_gpu import _execute_occupancy
    from test_quantile_gpu import _execute_quantile
    from test_track_gpu import _execute_track
    import test_bursts_gpu as tb
    import test_pulses_gpu as tp
    r = _f_request()
    n, W, lut, want = F_N, F_W, base._lut(), r["want"]
    data, nbytes = r["data"], r["data"].size
    out = {}
    plan = ctx.plan(F_FMT, n, r["win"], r["bn"], GAIN, RANGE, lut)
    peak_plan = ctx.plan(F_FMT, n, r["win"], r["bn"], GAIN, RANGE, lut, detector="peak")
    d_in = ctx.alloc(nbytes + 16)
    try:
        ctx.upload(d_in, data)
        d = plan.debug_launch(nbytes, W)
        assert d["kernel"] == "frames" and d["cu_count"] == cu and (d["gf"], d["groups"], d["grid"]) == launchref.launch(n, 256, W, cu), (what, d)

        def is_peak(d):
            assert (d["kernel"], d["peak_m"], d["cu_count"]) == ("frames_peak", 3, cu), (what, d)

        def is_index(d):
            assert d["kernel"] == "frames_index" and d["cu_count"] == cu, (what, d)

        out["image"] = base._run(ctx, plan, data, W, n, len(lut), False, lambda d: None, what)
        base._same(out["image"], want["image"], what + " image")
        out["peak"] = base._run(ctx, peak_plan, r["peak_data"], W, n, len(lut), False, is_peak, what)
        base._same(out["peak"], want["peak"], what + " peak")
        out["index"] = shapes.run(ctx, plan, data, W, n, len(lut), 0, is_index, what)
        shapes.same(out["index"], want["index"], what + " index")
        tmin, tmax = ss._Dev(ctx, 8 * n), ss._Dev(ctx, 8 * n)
        dens, pl = ss._Dev(ctx, 4 * n * len(lut)), ss._Dev(ctx, 8 * W * n)
        try:
            plan.execute_traces(d_in, nbytes, W, tmin.ptr, tmax.ptr)
            plan.execute_density(d_in, nbytes, W, dens.ptr)
            plan.execute_power(d_in, nbytes, W, pl.ptr)
            ctx.synchronize()
            out["traces"] = {"trace_min": tmin.read(np.float64, what), "trace_max": tmax.read(np.float64, what)}
            out["density"] = dens.read(np.uint32, what).reshape(n, len(lut))
            out["power"] = pl.read(np.float64, what).reshape(W, n)
        finally:
            for b in (tmin, tmax, dens, pl):
                b.free()
        tracesref.assert_same(out["traces"], want["traces"], what + " traces")
        assert np.array_equal(out["density"], want["density"].astype(np.uint32)), what + ": density differs"
        powerref.assert_same(out["power"], want["power"], what + " power")
        out["mean"] = _execute_mean(ctx, plan, d_in, nbytes, W, n, what)
        meanref.assert_same(out["mean"], want["mean"], what + " mean")
        out["blockmean"] = [_execute_blockmean(ctx, plan, d_in, nbytes, W, g, n, what) for g in F_GROUPS]
        for g, got_g, want_g in zip(F_GROUPS, out["blockmean"], want["blockmean"]):
            blockmeanref.assert_same(got_g, want_g, "%s blockmean of %d" % (what, g))
        out["bandpower"] = _execute_bandpower(ctx, plan, d_in, nbytes, W, r["bands"], what)
        bandref.assert_same(out["bandpower"], want["bandpower"], what + " bandpower")
        out["moments"] = _execute_moments(ctx, plan, d_in, nbytes, W, r["bands"], F_ORDER, what)
        momentref.assert_same(out["moments"], want["moments"], what + " moments")
        out["track"] = _execute_track(ctx, plan, d_in, nbytes, W, r["bands"], what)
        trackref.assert_same(out["track"], want["track"], what + " track")
        out["occupancy"] = _execute_occupancy(ctx, plan, d_in, nbytes, W, r["thr"], r["bands"], what)
        occref.assert_same(out["occupancy"], want["occupancy"], what + " occupancy")
        out["quantile"] = _execute_quantile(ctx, plan, d_in, nbytes, W, r["ranks"], what)
        quantileref.assert_same(out["quantile"], want["quantile"], what + " quantile")
        out["bursts"] = tb._execute_bursts(ctx, plan, d_in, nbytes, W, r["bands"], r["hi"], r["lo"], F_M, what)
        tb.assert_same(out["bursts"], want["bursts"], what + " bursts")
        out["pulses"] = tp._execute_pulses(ctx, plan, d_in, nbytes, W, r["bands"], r["hi"], r["lo"], F_M, what)
        tp.assert_same(out["pulses"], want["pulses"], what + " pulses")
        held, items = [], []
        try:
            for dj, w in zip(r["items"], F_BATCH):
                ptrs, blk = base._alloc_reply(ctx, w, n, len(lut), False)
                d_j = ctx.alloc(dj.size + 16)
                ctx.upload(d_j, dj)
                held.append((ptrs, blk, d_j))
                items.append((d_j, dj.size, w, ptrs))
            plan.execute_batch(items)
            ctx.synchronize()
            out["batch"] = [base._read_reply(ctx, ptrs, blk, w, n, len(lut), what) for (ptrs, blk, _), w in zip(held, F_BATCH)]
        finally:
            for ptrs, blk, d_j in held:
                base._free_reply(ctx, ptrs, blk)
                ctx.free(d_j)
        for j, (g, w) in enumerate(zip(out["batch"], want["batch"])):
            base._same(g, w, "%s batch item %d" % (what, j))
    finally:
        ctx.free(d_in)
        plan.close()
        peak_plan.close()
    assert set(out) == set(F_KINDS)
    return out


def _flat(v):
    """The arrays of a reply, in a fixed order, as bytes."""
    if isinstance(v, dict):
        return [a for k in sorted(v) for a in _flat(v[k])]
    if isinstance(v, (list, tuple)):
        return [a for x in v for a in _flat(x)]
    return [np.ascontiguousarray(v).view(np.uint8).reshape(-1)]


@pytest.mark.parametrize("cu", F_CUS, ids=["every_kind_cu%s" % (c or "_own") for c in F_CUS])
def test_no_reply_depends_on_the_cu_count(ctx, own, cu):
    what = "every_kind_cu%s" % (cu or "_own")
    with at(ctx, cu):
        assert _reported(ctx) == (cu or own)
        got = _f_replies(ctx, cu or own, what)
    first = FIRST.setdefault("replies", got)
    for kind in F_KINDS:
        a, b = _flat(got[kind]), _flat(first[kind])
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), "%s: %s differs from the first count's reply" % (what, kind)
    RAN.add(what)


def test_set_cu_count_refuses_and_restores(pkg, ctx, own):
    """-1 and one more than the part has are refused and change nothing; 0 puts the part's own count back."""
    try:
        ctx.set_cu_count(8)
        assert _reported(ctx) == 8
        for bad in (-1, own + 1):
            with pytest.raises(pkg.SpectroplotError) as e:
                ctx.set_cu_count(bad)
            assert e.value.status == -1 and _reported(ctx) == 8
        ctx.set_cu_count(own)
        assert _reported(ctx) == own
        ctx.set_cu_count(1)
        ctx.set_cu_count(0)
        assert _reported(ctx) == own
        other = pkg.Context(0)                      # an override is the context's own
        try:
            ctx.set_cu_count(16)
            assert _reported(other) == own and _reported(ctx) == 16
        finally:
            other.close()
    finally:
        ctx.set_cu_count(0)
    assert _reported(ctx) == own
    RAN.add("setter")


# ------------------------------------------------------------------------------------------------------------------ completeness
def expected_ids():
    ids = [_id("frames", cu, c) for cu, c in A_CASES] + [_id("peak", cu, c) for cu, c in B_PEAK]
    ids += [_id("batch", cu, BATCH[k]) for cu, k in B_BATCH] + [_id("index", cu, indexref.case_id(c)) for cu, c in C_INDEX]
    ids += [_id("traces", cu, _plane_id(c)) for cu, c in C_TRACES] + [_id("power", cu, _plane_id(c)) for cu, c in C_POWER]
    ids += [_id("scratch", SCRATCH_CU, c["id"]) for c in D_CASES] + ["mean_cu%d_n%d_W%d" % t for t in E_MEAN] + ["db_cu1_%d_%s" % t for t in E_DB]
    return ids + ["every_kind_cu%s" % (c or "_own") for c in F_CUS] + ["setter"]


def test_zz_every_case_ran(ctx, own):
    """Runs last in the module: every case ran (and passed); of the lattices, everything but the cells pinned as out of reach at 8 CUs;
    no override is left behind.  Prints the module's case count, total time and slowest case."""
    ids = expected_ids()
    assert len(set(ids)) == len(ids)
    assert RAN == set(ids), "%d of %d cases ran; missing %s" % (len(RAN), len(ids), sorted(set(ids) - RAN)[:8])
    for cu in FRAMES_CUS:
        ran = {launchref.case_id(c) for c in FRAMES if _id("frames", cu, c) in RAN}
        assert ran == {launchref.case_id(c) for c in FRAMES} - set(SKIPPED.get(("frames", cu), ())), cu
    for cu in LATTICE_CUS:
        ran = {launchref.case_id(c) for c in PEAK if _id("peak", cu, c) in RAN}
        assert ran == {launchref.case_id(c) for c in PEAK} - set(SKIPPED.get(("peak", cu), ())), cu
    assert sorted(SKIPPED) == [("frames", 8), ("peak", 8)] and (len(SKIPPED["frames", 8]), len(SKIPPED["peak", 8])) == (34, 5)
    assert _reported(ctx) == own
    slowest = max(TIMES, key=TIMES.get)
    print("\ntest_cu_counts_gpu: %d cases, %.1f s in all, slowest %s %.2f s" % (len(TIMES), sum(TIMES.values()), slowest, TIMES[slowest]))
