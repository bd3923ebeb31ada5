// sp_variance.hip — k_variance_accumulate and k_variance_finish (sp_kernel_variance.h) and their launchers (sp_launch.h): a device unit of
// its own beside sp_kernels.hip, whose set of kernels tests/test_isa_checks.py holds to its reference commit's.  Host code reaches the
// kernels through the launchers only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_variance.h"

namespace spk {

static_assert(spv::kSlots == 200, "a row's words: 66 + 132 cells and two counters");
static_assert(spv::kSlots * kVarRows * sizeof(unsigned long long) == 51200, "the LDS of a workgroup: three fit a CU's 160 KiB");

void variance_launch_shape(int n, long long frames, int cu_count, long long shape[3])
{
    const int pieces = variance_pieces(n, frames, cu_count);
    shape[0] = variance_bands(n), shape[1] = pieces, shape[2] = (frames + pieces - 1) / pieces;
}

void launch_variance_accumulate(const double *plane, int n, long long frames, unsigned long long *ws, int cu_count, hipStream_t stream)
{
    long long shape[3];
    variance_launch_shape(n, frames, cu_count, shape);
    hipLaunchKernelGGL(k_variance_accumulate, dim3((unsigned)shape[0], (unsigned)shape[1]), dim3(kVarThreads), 0, stream, plane, n, frames,
                       shape[2], ws);
}

void launch_variance_finish(const unsigned long long *ws, int n, int width, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_variance_finish, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, ws, n, width, out);
}

}  // namespace spk
