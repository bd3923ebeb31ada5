// sp_band_list.h - the bands of a launch as a kernel argument (k_band_sum of sp_kernel_band.h, k_track_max of sp_kernel_track.h).
#pragma once

#include <cstdint>

namespace spk {

constexpr int kBandMax = 64;        // SP_MAX_BANDS (sp_band.hip and sp_track.hip assert it)

// The bands of a launch as a kernel argument, 512 bytes: band b is the rows [y[2 b], y[2 b + 1]), checked by the host.
struct BandList {
    int32_t y[2 * kBandMax];
};

}  // namespace spk
