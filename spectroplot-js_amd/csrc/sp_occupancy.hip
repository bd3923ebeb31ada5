// sp_occupancy.hip — k_occupancy_count (sp_kernel_occupancy.h) and its launcher (sp_launch.h): a device unit of its own beside
// sp_kernels.hip, whose set of kernels tests/test_isa_checks.py holds to its reference commit's, as sp_band.hip and sp_track.hip are.
// Host code reaches the kernel through the launcher only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_occupancy.h"

namespace spk {

static_assert(kOccTileRows == SP_OCCUPANCY_TILE_ROWS, "the header names the kernel's tile");
static_assert(kBandMax <= 64, "a lane is a band");
void launch_occupancy_count(const double *plane, int n, long long frames, const double *threshold, const int32_t *bands, int count,
                            uint32_t *rows, uint32_t *out, long long stride, long long x_base, hipStream_t stream)
{
    const BandList list = band_list(bands, count);
    const unsigned pieces = (unsigned)((frames + kOccFrames - 1) / kOccFrames);
    const unsigned tiles = (unsigned)((n + kOccTileRows - 1) / kOccTileRows);
    hipLaunchKernelGGL(k_occupancy_count, dim3(pieces, tiles), dim3(kOccThreads), 0, stream, plane, n, frames,
                       (const unsigned long long *)threshold, list, count, rows, out, stride, x_base);
}

}  // namespace spk
