// sp_band.hip — k_band_sum<ORDER> (sp_kernel_band.h), the band sums and the moments, and its launcher (sp_launch.h): a device unit of
// its own beside sp_kernels.hip, whose set of kernels tests/test_isa_checks.py holds to its reference commit's.  Host code reaches the
// kernel through the launcher only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_band.h"

namespace spk {

static_assert(spm::kMaxRows == SP_MAX_N, "a row distance stays below SP_MAX_N: its square is a weight below 2^40");
static_assert(band_slots(0) == spx::kSlots && band_slots(0) * kBandFrames * sizeof(unsigned long long) == 4352, "the LDS of a workgroup at order 0");
static_assert(band_slots(spm::kMaxOrder) * kBandFrames * sizeof(unsigned long long) == 13184, "the LDS of a workgroup at order 2");

template <int ORDER>
static void launch(const double *plane, int n, long long frames, const BandList &list, int count, double *out, long long stride,
                   long long x_base, hipStream_t stream)
{
    const unsigned pieces = (unsigned)((frames + kBandFrames - 1) / kBandFrames);
    hipLaunchKernelGGL(k_band_sum<ORDER>, dim3(pieces, (unsigned)count), dim3(kBandThreads), 0, stream, plane, n, frames, list, out, stride,
                       x_base);
}

void launch_band_sum(const double *plane, int n, long long frames, const int32_t *bands, int count, int order, double *out, long long stride,
                     long long x_base, hipStream_t stream)
{
    const BandList list = band_list(bands, count);
    if (order == 0) launch<0>(plane, n, frames, list, count, out, stride, x_base, stream);
    else if (order == 1) launch<1>(plane, n, frames, list, count, out, stride, x_base, stream);
    else launch<2>(plane, n, frames, list, count, out, stride, x_base, stream);
}

}  // namespace spk
