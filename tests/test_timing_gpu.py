"""The timing pair of a context (sp_context_enable_timing, sp_context_last_kernel_ms) at every entry point on device operands: a call
that queues work leaves a pair that can be read once the stream has ended, a call that queues nothing or is refused leaves none.

One capture serves every case: CS16, n = 64, 32 frames one frame apart, a Hann window and a colour map of 16 entries.  Every output goes
to a device buffer of its size.  No lower bound above zero is asserted: the event clock's resolution is not something this project has
measured."""
import math

import numpy as np
import pytest

import siggen
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

GEN = {"kind": "trinoise", "seed": 2718, "step": 4099, "gshift": 10, "amp": 0.45, "namp": 0.03}
FMT, N, WIDTH, LUT_LEN = "CS16", 64, 32, 16
CB_HIST = 1000


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class _Rig:
    """The capture on the device, a sample plan and a peak plan for it, and one device buffer per output of every entry point."""

    def __init__(self, pkg, ctx):
        self.ctx = ctx
        data = siggen.generate(FMT, GEN, N * WIDTH)
        self.nbytes = int(data.size)
        self.bufs = []
        self.d_in = self.buf(self.nbytes)
        ctx.upload(self.d_in, data)
        win, weight = pkg.window("hann", N)
        lut = np.stack([np.linspace(0, 255, LUT_LEN).astype(np.uint8)] * 3, axis=1)
        self.plan = ctx.plan(FMT, N, win, 1.0 / weight, 3.0, 50.0, lut)
        self.peak_plan = ctx.plan(FMT, N, win, 1.0 / weight, 3.0, 50.0, lut, detector="peak")
        self.replies = [self.reply(), self.reply()]
        self.index = self.buf(WIDTH * N)
        self.density = self.buf(4 * N * LUT_LEN)
        self.trace_min, self.trace_max, self.mean = self.buf(8 * N), self.buf(8 * N), self.buf(8 * N)
        self.power, self.db = self.buf(8 * WIDTH * N), self.buf(8 * WIDTH * N)
        # the operands of the entry points that take a finished image or plane
        self.plan.execute_index(self.d_in, self.nbytes, WIDTH, index=self.index)
        self.plan.execute_power(self.d_in, self.nbytes, WIDTH, self.power)
        ctx.synchronize()

    def buf(self, nbytes):
        p = self.ctx.alloc(nbytes)
        self.ctx.memset(p, 0, nbytes)
        self.bufs.append(p)
        return p

    def reply(self):
        return {"rgba": self.buf(4 * WIDTH * N), "gauge_mins": self.buf(WIDTH), "gauge_maxs": self.buf(WIDTH), "gauge_amps": self.buf(WIDTH),
                "c_hist": self.buf(8 * LUT_LEN), "cb_hist": self.buf(8 * CB_HIST), "dbfs_minmax": self.buf(16)}

    def side(self, k=0):
        return {key: v for key, v in self.replies[k].items() if key != "rgba"}

    def close(self):
        self.plan.close()
        self.peak_plan.close()
        for p in self.bufs:
            self.ctx.free(p)


@pytest.fixture(scope="module")
def rig(pkg, ctx):
    r = _Rig(pkg, ctx)
    yield r
    r.close()


# entry point -> the call, on the rig's operands
CALLS = {
    "execute": lambda r: r.plan.execute(r.d_in, r.nbytes, WIDTH, **r.replies[0]),
    "execute_index": lambda r: r.plan.execute_index(r.d_in, r.nbytes, WIDTH, index=r.index, **r.side()),
    "execute_density": lambda r: r.plan.execute_density(r.d_in, r.nbytes, WIDTH, r.density),
    "execute_traces": lambda r: r.plan.execute_traces(r.d_in, r.nbytes, WIDTH, r.trace_min, r.trace_max),
    "execute_power": lambda r: r.plan.execute_power(r.d_in, r.nbytes, WIDTH, r.power),
    "power_to_db": lambda r: r.plan.power_to_db(r.power, WIDTH * N, r.db),
    "execute_mean": lambda r: r.plan.execute_mean(r.d_in, r.nbytes, WIDTH, r.mean),
    "power_mean": lambda r: r.ctx.power_mean(r.power, N, WIDTH, r.mean),
    "density_from_index": lambda r: r.ctx.density_from_index(r.index, N, WIDTH, False, LUT_LEN, r.density),
    "execute_batch": lambda r: r.plan.execute_batch([(r.d_in, r.nbytes, WIDTH, r.replies[0]), (r.d_in, r.nbytes, WIDTH, r.replies[1])]),
}
SCRATCH_TOO = ["execute", "execute_traces", "execute_power", "execute_mean"]


def _no_pair(pkg, ctx):
    with pytest.raises(pkg.SpectroplotError):
        ctx.last_kernel_ms()


def _leaves_a_pair(pkg, ctx, rig, entry):
    ctx.enable_timing(True)   # (clears the pair)
    _no_pair(pkg, ctx)
    CALLS[entry](rig)
    ctx.synchronize()
    ms = ctx.last_kernel_ms()
    assert math.isfinite(ms) and ms >= 0, (entry, ms)


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_a_device_entry_point_leaves_a_timing_pair(pkg, ctx, rig, entry):
    try:
        _leaves_a_pair(pkg, ctx, rig, entry)
    finally:
        ctx.enable_timing(False)


@pytest.mark.parametrize("entry", SCRATCH_TOO)
def test_a_device_entry_point_leaves_a_timing_pair_on_the_scratch_kernels(pkg, ctx, rig, entry):
    rig.plan.force_kernel("scratch")
    try:
        _leaves_a_pair(pkg, ctx, rig, entry)
    finally:
        rig.plan.force_kernel("auto")
        ctx.enable_timing(False)


def test_a_power_request_of_no_frames_leaves_no_timing_pair(pkg, ctx, rig):
    try:
        ctx.enable_timing(True)
        rig.plan.execute_power(rig.d_in, rig.nbytes, 0, rig.power)
        ctx.synchronize()
        _no_pair(pkg, ctx)
    finally:
        ctx.enable_timing(False)


def test_a_refused_traces_request_leaves_no_timing_pair(pkg, ctx, rig):
    try:
        ctx.enable_timing(True)
        with pytest.raises(pkg.SpectroplotError) as e:
            rig.peak_plan.execute_traces(rig.d_in, rig.nbytes, WIDTH, rig.trace_min, rig.trace_max)
        assert e.value.status == pkg.binding.SP_ERR_UNSUPPORTED
        ctx.synchronize()
        _no_pair(pkg, ctx)
    finally:
        ctx.enable_timing(False)
