"""Whole-reply parity of the indexed image at every launch shape of k_frames_index.

Each case of tests/indexref.py's lattice - every built (n, loader) once, over which the (gf, regime) cells, L/R split, layout and the
fast / slow write-out (slow by width: W % 16 != 0 with W % 4 == 0 or not; slow by pointer: the image 1 or 4 bytes off 16-byte
alignment) rotate - is ONE launch of sp_plan_execute_index whose shape is confirmed through sp_plan_debug_index_launch before anything
is rendered.  The reply is compared whole and bit for bit, no tolerance, with the oracle (the LUT is injective with R = index, so the
expected index image is the oracle's rgba[..., 0]) and with the same request forced onto render_extract.  Inputs, garbage-filled
outputs and guard bytes as in tests/test_launch_shapes_gpu.py, whose helpers this module uses.  The last test asserts the lattice ran."""
import numpy as np
import pytest

import indexref
import launchref
import test_launch_shapes_gpu as base
from oracle import pyoracle

pytestmark = pytest.mark.gpu

CASES = indexref.lattice()
RAN = set()
GUARD = base.GUARD
pkg, ctx, cu = base.pkg, base.ctx, base.cu   # (module-scoped fixtures, instantiated for this module)


def _alloc(ctx, W, n, L, off):
    """Device buffers of an indexed reply, all garbage; the index image between guards, `off` bytes past 16-byte alignment."""
    size = W * n
    blk = ctx.alloc(size + 2 * GUARD + 16)
    ctx.memset(blk, 0xAB, size + 2 * GUARD + 16)
    sizes = {"gauge_mins": W, "gauge_maxs": W, "gauge_amps": W, "c_hist": 8 * L, "cb_hist": 8000, "dbfs_minmax": 16}
    ptrs = {k: ctx.alloc(max(v, 16)) for k, v in sizes.items()}
    for k, v in sizes.items():
        ctx.memset(ptrs[k], 0xAB, max(v, 16))
    ptrs["index"] = blk + GUARD + off
    assert blk % 16 == 0
    return ptrs, blk


def _read(ctx, ptrs, blk, W, n, L, what):
    size = W * n
    whole = ctx.download(blk, size + 2 * GUARD + 16)
    off = ptrs["index"] - blk
    assert (whole[:off] == 0xAB).all() and (whole[off + size:] == 0xAB).all(), what + ": bytes around the index image were written"
    out = {"index": whole[off:off + size]}
    for k in ("gauge_mins", "gauge_maxs", "gauge_amps"):
        out[k] = ctx.download(ptrs[k], W) if W else np.zeros(0, np.uint8)
    out["c_hist"] = ctx.download(ptrs["c_hist"], 8 * L, np.uint64)
    out["cB_hist"] = ctx.download(ptrs["cb_hist"], 8000, np.uint64)
    out["mm"] = ctx.download(ptrs["dbfs_minmax"], 16, np.uint64)
    return out


def _free(ctx, ptrs, blk):
    for k, p in ptrs.items():
        if k != "index":
            ctx.free(p)
    ctx.free(blk)


def same(got, want, what):
    """The whole indexed reply against the oracle's reply (rendered with base._lut())."""
    exp = indexref.expected_index(want)
    if not np.array_equal(got["index"], exp):
        bad = np.flatnonzero(got["index"] != exp)
        raise AssertionError("%s: index differs in %d places, first at %d" % (what, bad.size, bad[0]))
    assert np.array_equal(np.bincount(got["index"], minlength=len(want["c_hist"])), want["c_hist"]), what + ": bincount(index) != c_hist"
    base._same(dict(got, rgba=want["rgba"]), want, what)


def run(ctx, plan, data, W, n, L, off, check_launch, what):
    ptrs, blk = _alloc(ctx, W, n, L, off)
    d_in = ctx.alloc(data.size + 16)
    try:
        check_launch(plan.debug_index_launch(data.size, W, ptrs["index"]))
        ctx.upload(d_in, data)
        plan.execute_index(d_in, data.size, W, **ptrs)
        ctx.synchronize()
        return _read(ctx, ptrs, blk, W, n, L, what)
    finally:
        _free(ctx, ptrs, blk)
        ctx.free(d_in)


@pytest.fixture(scope="module")
def ahead(cu):
    pyoracle.lib()

    def make(c):
        n = c["n"]
        W = indexref.choose_width(n, cu, c["gf"], c["regime"], c["writeout"])
        assert W is not None, "the rule allows no width for %r on %d CUs" % (c, cu)
        data = base._capture(c["fmt"], n, W, c["gf"], "overlap")
        win, weight = pyoracle.window("blackmanHarris" if c["wf"] else "hann", n)
        want = pyoracle.render(c["fmt"], data, n, win, 1.0 / weight, base.GAIN, base.RANGE, base._lut(), W, c["ch"], c["wf"])
        return W, data, win, weight, want

    a = base._Ahead(CASES, make)
    yield a
    a.pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[indexref.case_id(c) for c in CASES])
def test_k_frames_index_whole_reply(pkg, ctx, cu, ahead, k):
    c = CASES[k]
    what = indexref.case_id(c)
    n = c["n"]
    W, data, win, weight, want = ahead.get(k)
    assert data.size <= base.MAX_CAPTURE
    lut = base._lut()
    fast = c["writeout"] == "fast"

    def frames_launch(d):
        assert d["kernel"] == "frames_index" and d["cu_count"] == cu and d["log2n"] == n.bit_length() - 1, d
        assert d["gf"] == c["gf"] and d["groups"] == -(-W // c["gf"]) and d["grid"] == launchref.grid_for(d["groups"], cu), d
        assert launchref.regime_of(d["groups"], d["grid"]) == c["regime"] and d["groups"] % 8 != 0, d
        assert d["prefetch"] == c["loader"] and d["rgba_fast"] == int(fast) and d["channel_mode"] == int(c["ch"]), d
        assert 0 < d["lds_bytes"] <= 160 * 1024, d

    def extract_launch(d):
        assert d["kernel"] == "scratch_radix2" and d["rgba_fast"] == 0, d

    plan = ctx.plan(c["fmt"], n, win, 1.0 / weight, base.GAIN, base.RANGE, lut, c["ch"], c["wf"])
    try:
        assert plan.index_kernel_name_for(data.size, W) == "frames_index"
        got = run(ctx, plan, data, W, n, len(lut), indexref.misalign(c["writeout"]), frames_launch, what)
        same(got, want, "%s W=%d" % (what, W))
        plan.force_kernel("scratch")
        assert plan.index_kernel_name_for(data.size, W) == "render_extract"
        got = run(ctx, plan, data, W, n, len(lut), indexref.misalign(c["writeout"]), extract_launch, what)
        same(got, want, "%s W=%d render_extract" % (what, W))
    finally:
        plan.close()
    RAN.add(what)


def test_zz_the_whole_lattice_ran(cu):
    """Runs last in the module: every case of the lattice has run (and passed) on this part; the n = 1024 group of 32 is among them."""
    ids = {indexref.case_id(c) for c in CASES}
    assert len(ids) == len(CASES) == 6 * len(launchref.SIZES)
    assert RAN == ids, "%d of %d cases ran on %d CUs; missing %s" % (len(RAN), len(ids), cu, sorted(ids - RAN)[:8])
    assert any(c["n"] == 1024 and c["gf"] == 32 for c in CASES)
    assert {c["writeout"] for c in CASES} == {"fast", "w4", "w1", "p1", "p4"}
    assert {(c["ch"], c["wf"]) for c in CASES} == {(False, False), (False, True), (True, False), (True, True)}
