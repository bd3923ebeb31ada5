"""Expected power planes of a request (include/spectroplot_hip.h, sp_plan_execute_power), from the EXISTING oracle only: the abs2 and db
planes of pyoracle.render(..., planes=True), whose columns are in bin order, permuted to image row order (worker.js:90) with
tracesref.rows.  Test infrastructure, not a test."""
import numpy as np

import tracesref
from oracle import pyoracle

_LUT = tracesref._LUT      # the colours do not reach a plane


def expected(fmt, data, n, windowc, block_norm, gain, rng, width, channel_mode=False):
    """{"power": f64 [width, n], "db": f64 [width, n]} in row order, and the oracle's whole reply under "ref"."""
    ref = pyoracle.render(fmt, data, n, windowc, block_norm, gain, rng, _LUT, width, channel_mode, False, planes=True)
    y = tracesref.rows(n)
    power, db = np.empty((width, n)), np.empty((width, n))
    power[:, y] = ref["abs2"]
    db[:, y] = ref["db"]
    return {"power": power, "db": db, "ref": ref}


def same_plane(a, b):
    """Two f64 planes agree: the same shape, NaN at the same positions, the same bits everywhere else.  Which NaN a NaN is (payload,
    sign) is the one thing left uncompared."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not (na == nb).all():
        return False
    return bool((a.view(np.uint64)[~na] == b.view(np.uint64)[~na]).all())


def assert_same(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %r, want %r" % (what, got.shape, want.shape)
    if same_plane(got, want):
        return
    na, nb = np.isnan(got), np.isnan(want)
    bad = np.argwhere((na != nb) | (~na & ~nb & (got.view(np.uint64) != want.view(np.uint64))))
    x, y = bad[0]
    raise AssertionError("%s: the plane differs in %d of %d values, first at frame %d row %d: got %r, want %r"
                         % (what, len(bad), want.size, x, y, got[x, y], want[x, y]))


def assert_telling(plane, what=""):
    """A reference plane against which a permutation or stride mistake cannot hide: no NaN, no zero, mostly distinct values."""
    assert not np.isnan(plane).any(), "%s: the reference plane holds NaN" % what
    assert not (plane == 0.0).any(), "%s: the reference plane holds zeros" % what
    assert len(np.unique(plane)) >= plane.size // 2, "%s: the reference plane repeats its values" % what
