"""What a density reply (sp_*_density: per-row colour-index counts) must hold, from what the tree already has: the oracle's reply
rendered with an injective LUT whose R channel is the index (tests/indexref.py), un-laid by the layout's pixel formula and counted per
image row with numpy.  Test infrastructure, not a test."""
import numpy as np

import indexref


def rows_of(index, n, width, waterfall):
    """The index image as [n image rows, width frames]: pixel j = x + width * y of the spectrogram layout, j = n * (width - 1 - x) +
    (n - 1 - y) of the waterfall layout (include/spectroplot_hip.h, sp_plan_execute_index)."""
    index = np.asarray(index, np.uint8).reshape(-1)
    assert index.size == n * width
    if not waterfall:
        return index.reshape(n, width)
    return index.reshape(width, n)[::-1, ::-1].T


def count_image(index, n, width, waterfall, lut_len):
    """density[y][g] = #{x : index(x, y) == g} of a raw index image; bytes >= lut_len are counted nowhere.  -> uint32 [n, lut_len]"""
    rows = rows_of(index, n, width, waterfall).astype(np.int64)
    out = np.zeros((n, 256), np.int64)
    if width:
        np.add.at(out, (np.repeat(np.arange(n), width), rows.reshape(-1)), 1)
    assert int(out.sum()) == n * width
    return out[:, :lut_len].astype(np.uint32)


def expected(want, n, lut_len, width, waterfall):
    """The density of the request whose oracle reply (LUT: R channel = index) is `want`."""
    rows = rows_of(indexref.expected_index(want), n, width, waterfall)
    out = np.stack([np.bincount(r, minlength=lut_len) for r in rows]) if width else np.zeros((n, lut_len), np.int64)
    assert out.shape == (n, lut_len)
    return out.astype(np.uint32)
