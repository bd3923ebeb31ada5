// sp_track.hip — k_track_max (sp_kernel_track.h) and its launcher (sp_launch.h): a device unit of its own beside sp_kernels.hip, whose
// set of kernels tests/test_isa_checks.py holds to its reference commit's, as sp_band.hip is.  Host code reaches the kernel through the
// launcher only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_track.h"

namespace spk {

void launch_track_max(const double *plane, int n, long long frames, const int32_t *bands, int count, int32_t *row, double *peak,
                      long long stride, long long x_base, hipStream_t stream)
{
    const BandList list = band_list(bands, count);
    const unsigned pieces = (unsigned)((frames + kTrackFrames - 1) / kTrackFrames);
    hipLaunchKernelGGL(k_track_max, dim3(pieces, (unsigned)count), dim3(kTrackThreads), 0, stream, plane, n, frames, list, row, peak, stride,
                       x_base);
}

}  // namespace spk
