"""CPU: the slice layout of a sliced render (sp_debug_slice_layout, spgeo::SliceLayout) against the reference's own formulas,
sliceWidth = ~~(width / renderWorkerCount) (lib/spectroplot.js:1208) and putImageData(image, waterfall ? 0 : offset,
waterfall ? width - sliceWidth - offset : 0) with offset = i * sliceWidth (lib/spectroplot.js:1221, 1244), written out here in bytes of
the RGBA canvas.  No device: the layout is host arithmetic.  What the group tests check through images, this checks through geometry:
the strips' bands are disjoint, lie inside the image and, together with the rectangle no strip draws, cover it exactly."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

NS = (2, 64, 8192)
COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 64)
BIG_ODD = 100003


@pytest.fixture(scope="module")
def lib():
    L = load_package().Library.get().L
    L.sp_debug_slice_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_size_t)]
    return L


def widths(count):
    return sorted(set([0, 1, count - 1, count, count + 1, 5 * count, BIG_ODD]))


def layout(lib, n, width, count, waterfall):
    buf = (C.c_int64 * (10 + 2 * count))()
    used = C.c_size_t()
    rc = lib.sp_debug_slice_layout(n, width, count, int(waterfall), buf, len(buf), C.byref(used))
    assert rc == 0 and used.value == len(buf), (rc, used.value)
    v = list(buf)
    keys = ("slice_width", "strip_bytes", "rest", "band_pitch", "band_row_bytes", "band_rows", "rest_offset", "rest_pitch", "rest_row_bytes",
            "rest_rows")
    d = dict(zip(keys, v[:10]))
    d["band_offset"] = v[10::2]
    d["gauge_offset"] = v[11::2]
    return d


def reference(n, width, count, waterfall):
    """The canvas is width x n pixels (spectrogram: one column per frame) or n x width (waterfall: one row per frame), 4 bytes a pixel.
    Returns sliceWidth and the top-left pixel (x, y) of every strip, as the reference puts them."""
    slice_width = int(width / count)                                   # ~~(width / renderWorkerCount)               :1208
    at = []
    for i in range(count):
        offset = i * slice_width                                       # offset: i * sliceWidth                      :1221
        at.append((0, width - slice_width - offset) if waterfall else (offset, 0))                                 # :1244
    return slice_width, at


def rect_segments(offset, pitch, row_bytes, rows):
    """The byte intervals of a rectangle, merged where rows touch."""
    if row_bytes == 0 or rows == 0:
        return []
    if rows == 1 or pitch == row_bytes:
        return [(offset, offset + row_bytes * rows)]
    return [(offset + pitch * y, offset + pitch * y + row_bytes) for y in range(rows)]


def check_point(lib, n, width, count, waterfall, brute):
    d = layout(lib, n, width, count, waterfall)
    sw, at = reference(n, width, count, waterfall)
    canvas_w = n if waterfall else width                               # pixels per canvas row
    image = 4 * width * n
    assert d["slice_width"] == sw and d["strip_bytes"] == 4 * sw * n and d["rest"] == width - sw * count
    for r in range(count):
        assert d["band_offset"][r] == 4 * (canvas_w * at[r][1] + at[r][0]), (n, width, count, waterfall, r)
        assert d["gauge_offset"][r] == r * sw
    # a strip is sliceWidth x n pixels (spectrogram) or n x sliceWidth (waterfall: newImageData(data, height), :1241); its band is the
    # strip's rows in the canvas, row by row, or in one piece where those rows follow each other
    strip_w, strip_h = (n, sw) if waterfall else (sw, n)
    bands = [(d["band_offset"][r], d["band_pitch"], d["band_row_bytes"], d["band_rows"]) for r in range(count)] if sw else []
    for off, pitch, row_bytes, rows in bands:
        if rows == strip_h:
            assert row_bytes == 4 * strip_w and (rows == 1 or pitch == 4 * canvas_w)
        else:
            assert rows == 1 and row_bytes == 4 * strip_w * strip_h and strip_w == canvas_w
        assert 0 <= off and off + pitch * (rows - 1) + row_bytes <= image, "band outside the image"
    rest = (d["rest_offset"], d["rest_pitch"], d["rest_row_bytes"], d["rest_rows"]) if d["rest"] else None
    # exact cover, by intervals.  Column bands and a column rest share pitch and rows: their first rows must tile one canvas row.
    rects = bands + ([rest] if rest else [])
    if waterfall or not rects:
        segs = sorted(s for rc in rects for s in rect_segments(*rc))
        whole = image
    else:
        assert all(rc[1] == 4 * width and rc[3] == n for rc in rects)
        segs = sorted((rc[0], rc[0] + rc[2]) for rc in rects if rc[2])
        whole = 4 * width
    pos = 0
    for a, b in segs:
        assert a == pos, ("gap or overlap", n, width, count, waterfall, a, pos)
        pos = b
    assert pos == whole, ("the image is not covered", n, width, count, waterfall, pos, whole)
    if brute:                                                          # ... and byte by byte where the image is small
        hits = np.zeros(image, np.uint8)
        for off, pitch, rb, rows in rects:
            for y in range(rows):
                hits[off + pitch * y:off + pitch * y + rb] += 1
        assert (hits == 1).all(), (n, width, count, waterfall)


@pytest.mark.parametrize("waterfall", [False, True], ids=["spectrogram", "waterfall"])
def test_bands_and_rest_tile_the_image_as_the_reference_places_them(lib, waterfall):
    points = 0
    for n in NS:
        for count in COUNTS:
            for width in widths(count):
                check_point(lib, n, width, count, waterfall, brute=n <= 64 and 4 * width * n <= (1 << 20))
                points += 1
    assert points >= 3 * 9 * 6


def test_slice_width_of_the_golden_worker_cases(lib, golden):
    seen = 0
    for c in golden.spec["worker_cases"]:
        e = golden.expected[c["name"]]
        if "merged" not in e or "slice_width" not in e["merged"]:
            continue
        d = layout(lib, c["n"], c["width"], c["slices"], c["waterfall"])
        assert d["slice_width"] == e["merged"]["slice_width"], c["name"]
        seen += 1
    assert seen >= 1


def test_rejects_what_it_cannot_lay_out(lib):
    buf = (C.c_int64 * 16)()
    used = C.c_size_t()
    for n, width, count in ((0, 8, 2), (64, -1, 2), (64, 8, 0)):
        assert lib.sp_debug_slice_layout(n, width, count, 0, buf, len(buf), C.byref(used)) == -1
    assert lib.sp_debug_slice_layout(64, 8, 4, 0, buf, 4, C.byref(used)) == -1 and used.value == 18
