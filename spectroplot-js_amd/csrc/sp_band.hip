// sp_band.hip — k_band_sum (sp_kernel_band.h) and its launcher (sp_launch.h): a device unit of its own beside sp_kernels.hip, whose set
// of kernels tests/test_isa_checks.py holds to its reference commit's.  Host code reaches the kernel through the launcher only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_band.h"

namespace spk {

static_assert(kBandMax == SP_MAX_BANDS, "BandList holds SP_MAX_BANDS bands");
void launch_band_sum(const double *plane, int n, long long frames, const int32_t *bands, int count, double *band, long long stride,
                     long long x_base, hipStream_t stream)
{
    BandList list{};
    for (int k = 0; k < 2 * count; k++) list.y[k] = bands[k];
    const unsigned pieces = (unsigned)((frames + kBandFrames - 1) / kBandFrames);
    hipLaunchKernelGGL(k_band_sum, dim3(pieces, (unsigned)count), dim3(kBandThreads), 0, stream, plane, n, frames, list, band, stride, x_base);
}

}  // namespace spk
