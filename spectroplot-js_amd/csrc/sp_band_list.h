// sp_band_list.h - the bands of a launch as a kernel argument (k_band_sum of sp_kernel_band.h, k_track_max of sp_kernel_track.h,
// k_occupancy_count of sp_kernel_occupancy.h), and how their launchers fill it.
#pragma once

#include <cstdint>

#include "../../include/spectroplot_hip.h"

namespace spk {

constexpr int kBandMax = 64;
static_assert(kBandMax == SP_MAX_BANDS, "BandList holds SP_MAX_BANDS bands");

// The bands of a launch as a kernel argument, 512 bytes: band b is the rows [y[2 b], y[2 b + 1]), checked by the host.
struct BandList {
    int32_t y[2 * kBandMax];
};

// the `count` <= kBandMax bands of the host array `bands`, the rest zero
inline BandList band_list(const int32_t *bands, int count)
{
    BandList list{};
    for (int k = 0; k < 2 * count; k++) list.y[k] = bands[k];
    return list;
}

}  // namespace spk
