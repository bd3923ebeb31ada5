// slice_layout_walk.cpp — spgeo::SliceLayout and sp_debug_slice_layout over the grid of tests/test_slice_layout_cpu.py, as a program of
// its own so that the host arithmetic can run under the sanitizers (`make -C tests/cpp slice_layout_walk` builds and runs it).
// Every point: the bands and the rest, as rectangles of bytes, tile the image exactly (lib/spectroplot.js:1208, 1244).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/spectroplot_hip.h"
#include "../../spectroplot-js_amd/csrc/sp_geometry.h"

static int walk_point(int32_t n, int32_t width, int32_t count, int32_t waterfall)
{
    std::vector<int64_t> v(10 + 2 * (size_t)count);
    size_t used = 0;
    if (sp_debug_slice_layout(n, width, count, waterfall, v.data(), v.size(), &used) != SP_OK || used != v.size()) return 1;
    size_t small = 0;
    if (sp_debug_slice_layout(n, width, count, waterfall, v.data(), 3, &small) != SP_ERR_INVALID_ARG || small != used) return 2;
    const spgeo::SliceLayout s(n, width, count, waterfall != 0);
    if ((int64_t)s.slice_width != v[0] || (int64_t)s.strip_bytes() != v[1] || (int64_t)s.rest != v[2]) return 3;
    // first-row intervals of every rectangle: row bands are one row of the whole image, column bands share pitch and rows
    const size_t whole = waterfall ? s.image_bytes() : 4 * s.width;
    std::vector<std::pair<size_t, size_t>> seg;
    if (!waterfall && (s.band_pitch() != whole || s.band_rows() != s.n || s.rest_pitch() != whole || s.rest_rows() != s.n)) return 9;
    for (size_t r = 0; r < s.count && s.slice_width; r++) {
        if ((int64_t)s.band_offset(r) != v[10 + 2 * r] || (int64_t)s.gauge_offset(r) != v[11 + 2 * r]) return 4;
        if (s.band_offset(r) + s.band_pitch() * (s.band_rows() - 1) + s.band_row_bytes() > s.image_bytes()) return 5;
        seg.emplace_back(s.band_offset(r), s.band_offset(r) + s.band_row_bytes());
    }
    if (s.rest) {
        if (s.rest_offset() + s.rest_pitch() * (s.rest_rows() - 1) + s.rest_row_bytes() > s.image_bytes()) return 6;
        seg.emplace_back(s.rest_offset(), s.rest_offset() + s.rest_row_bytes());
    }
    std::sort(seg.begin(), seg.end());
    size_t pos = 0;
    for (const auto &ab : seg) {
        if (ab.first != pos) return 7;
        pos = ab.second;
    }
    return pos == (seg.empty() ? 0 : whole) && (!seg.empty() || s.image_bytes() == 0) ? 0 : 8;
}

int main()
{
    int points = 0;
    for (int32_t n : {2, 64, 8192})
        for (int32_t count : {1, 2, 3, 4, 5, 6, 7, 8, 64})
            for (int32_t width : {0, 1, count - 1, count, count + 1, 5 * count, 100003})
                for (int32_t waterfall : {0, 1}) {
                    const int bad = walk_point(n, width, count, waterfall);
                    if (bad) {
                        printf("slice layout n=%d width=%d count=%d waterfall=%d: check %d failed\n", n, width, count, waterfall, bad);
                        return 1;
                    }
                    points++;
                }
    printf("slice layout: %d points ok\n", points);
    return 0;
}
