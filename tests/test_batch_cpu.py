"""Batches without a device: the new entry points are exported and check their arguments, the host's work list (sp_debug_batch_plan)
covers every frame of every item once with launch_frames' rules, and the batch kernels' prefetching variants use no scratch memory
(tests/test_isa_checks.py compares the instruction streams of k_frames and k_frames_batch with their reference commits)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import isa
from launchref import batch_gf as _batch_gf, group_frames_for as _group_frames_for  # noqa: F401
from __graft_entry__ import build, load_package

SW = [1, 1, 2, 2, 3, 3, 4, 4, 8, 8, 16, 16, 8, 16]      # bytes per complex sample, enum sp_format order
ELEM = [1, 1, 1, 1, 1, 1, 2, 2, 4, 4, 8, 8, 4, 8]        # element size of the typed view


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


class _Reply(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rgba", "gmin", "gmax", "gamp", "c", "cb", "mm")]


class _Item(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("nbytes", C.c_size_t), ("width", C.c_int32), ("reserved", C.c_int32), ("reply", _Reply)]


def test_batch_symbols_and_argument_errors(pkg):
    lib = C.CDLL(pkg.lib_path())
    for name in ("sp_plan_execute_batch", "sp_render_batch", "sp_debug_batch_plan"):
        assert hasattr(lib, name), name
    lib.sp_plan_execute_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.sp_render_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    items = (_Item * 2)()
    for f in (lambda it, c: lib.sp_plan_execute_batch(None, it, c), lambda it, c: lib.sp_render_batch(None, None, it, c)):
        assert f(items, -1) == -1                       # count < 0
        assert f(None, 1) == -1                         # items == NULL with count > 0
    dev = pkg.Library.get().device_count()
    want = -5 if dev == 0 else -1                       # no context: SP_ERR_NO_DEVICE without a device
    assert lib.sp_plan_execute_batch(None, items, 2) == want
    assert lib.sp_render_batch(None, None, items, 2) == want
    with pytest.raises(pkg.SpectroplotError):
        pkg.binding.debug_batch_plan("cu8", 512, 256, 256, [100], [-1])


def _launch(fmt, n, nbytes, w):
    """launch_frames' loader choice for one item: 0 prefetching, 1 generic, 3 nothing to render."""
    if w == 0:
        return 3
    sw = SW[fmt]
    sc = nbytes / sw
    if w == 1:
        stride, ib = 0.0, n * sw <= nbytes
    else:
        stride = (sc - n) / (w - 1)
        ib = False
        if stride >= 0 and np.isfinite(stride) and 0.5 + stride * (w - 1) < 2147483647.0:
            ib = (int(0.5 + stride * (w - 1)) + n) * sw <= nbytes
    pf = ib and (sw <= 4 or sw == 8)
    if pf and sw == 3 and not (w >= 2 and int(0.5 + stride * (w - 1)) >= 1):
        pf = False
    return 0 if pf else 1


def test_batch_work_list_on_random_item_lists(pkg):
    rng = np.random.default_rng(2026)
    checked = 0
    for case in range(3000):
        fmt = int(rng.integers(0, 14))
        n = 1 << int(rng.choice(list(range(1, 14)) + [6, 7, 8, 9] * 4))   # mostly the sizes the batch kernel takes
        cu = int(rng.choice([8, 64, 256]))
        count = int(rng.integers(1, 40))
        widths, nbytes = [], []
        for _ in range(count):
            w = int(rng.choice([0, 1, int(rng.integers(2, 5000))]))
            kind = rng.integers(0, 3)
            if kind == 0:
                samples = int(rng.integers(0, n))                          # shorter than a frame
            elif kind == 1:
                samples = n + max(w - 1, 0) * int(rng.integers(n + 1, 3 * n))   # stride above n
            else:
                samples = int(rng.integers(n, 4 * n + w * n // 2 + 1))
            nb = samples * SW[fmt] // ELEM[fmt] * ELEM[fmt]
            widths.append(w)
            nbytes.append(nb)
        gf, grids, groups, rows = pkg.binding.debug_batch_plan(fmt, n, 256, cu, nbytes, widths)
        if not 64 <= n <= 512:                              # (k_frames_batch is built for n <= 512: larger plans go item by item)
            assert gf == 0 and all(r[0] == 2 for r in rows), (fmt, n)
            continue
        assert gf == _batch_gf(n, sum(widths), cu), (fmt, n, cu)
        per = {0: [], 1: []}
        for k, (lw, first, cnt) in enumerate(rows):
            assert lw == _launch(fmt, n, nbytes[k], widths[k]), (case, k, fmt, n, nbytes[k], widths[k])
            if lw == 3:
                assert cnt == 0
                continue
            assert cnt == -(-widths[k] // gf)                # every frame in exactly one group, the last one possibly partial
            per[lw].append((first, cnt))
        for lw in (0, 1):
            spans = sorted(per[lw])
            at = 0
            for first, cnt in spans:                         # an item's groups are its own and follow the previous item's
                assert first == at
                at += cnt
            assert at == groups[lw]
            assert grids[lw] == (0 if at == 0 else (min(at, cu) + 7) // 8 * 8)
        checked += 1
    assert checked > 1500


def test_batch_kernels_prefetching_iq_variants_use_no_scratch_memory():
    """Every I/Q prefetching variant of k_frames_batch has a private segment of zero bytes and no spilled VGPR, as every k_frames one
    (test_isa_checks.py).  The batch kernel is built for n = 64 ... 512 only; no object holds one for a larger n."""
    seen = 0
    for o in isa.frame_objs():
        for blk in isa.notes(o).split(".name:")[1:]:
            m = re.match(r"\s*_ZN4spk214k_frames_batchILi(\d+)ELb([01])ELi(\d+)E", blk)
            if not m:
                continue
            assert int(m.group(1)) <= 9, m.group(0)
            if m.group(2) == "1" or m.group(3) == "0":
                continue
            seen += 1
            priv = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
            spill = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1))
            assert priv == 0 and spill == 0, (m.group(0), priv, spill)
    assert seen == 4 * 5           # four sizes x five prefetch widths
