// sp_blockmean.hip — k_blockmean and k_power_to_index (sp_kernel_blockmean.h) and their launchers (sp_launch.h): a device unit of its
// own beside sp_kernels.hip, whose set of kernels tests/test_isa_checks.py holds to its reference commit's.  The carried path of a
// block mean runs k_mean_accumulate and k_mean_finish of sp_kernels.hip, unchanged.  Host code reaches the kernels through the
// launchers only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_blockmean.h"

namespace spk {

void blockmean_launch_shape(int n, long long frames, long long group, int cu_count, long long shape[3])
{
    const long long columns = spbm::columns(frames, group), bands = ((long long)n + kBlockMeanRows - 1) / kBlockMeanRows;
    // about eight workgroups per CU where there are columns enough: a workgroup is one column at a time, and a short one is brief
    long long pieces = (8ll * cu_count + bands - 1) / bands;
    if (pieces > columns) pieces = columns;
    if (pieces > 65535) pieces = 65535;
    if (pieces < 1) pieces = 1;
    const long long per = (columns + pieces - 1) / pieces;
    shape[0] = bands;
    shape[1] = per > 0 ? (columns + per - 1) / per : 1;
    shape[2] = per;
}

void launch_blockmean(const double *plane, int n, long long frames, long long group, double *out, int cu_count, hipStream_t stream)
{
    long long shape[3];
    blockmean_launch_shape(n, frames, group, cu_count, shape);
    hipLaunchKernelGGL(k_blockmean, dim3((unsigned)shape[0], (unsigned)shape[1]), dim3(kBlockMeanThreads), 0, stream, plane, n, frames, group,
                       spbm::columns(frames, group), shape[2], out);
}

int launch_power_to_index(const double *power, int n, int width, bool waterfall, const double *gray_edge, int lut_len, uint8_t *index,
                          hipStream_t stream)
{
    const long long bands = ((long long)n + kIndexTile - 1) / kIndexTile, tiles = ((long long)width + kIndexTile - 1) / kIndexTile;
    if (lut_len < 1 || lut_len > 256 || bands > 65535) return SP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_power_to_index, dim3((unsigned)tiles, (unsigned)bands), dim3(kIndexThreads), 0, stream, power, n, width,
                       waterfall ? 1 : 0, gray_edge, lut_len, index);
    return SP_OK;
}

}  // namespace spk
