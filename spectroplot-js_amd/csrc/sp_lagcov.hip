// sp_lagcov.hip — k_lagcov_accumulate and k_lagcov_finish (sp_kernel_lagcov.h) and their launchers (sp_launch.h): a device unit of its
// own beside sp_kernels.hip, whose set of kernels tests/test_isa_checks.py holds to its reference commit's.  Host code reaches the
// kernels through the launchers only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_lagcov.h"

namespace spk {

static_assert(spl::kSlots == 200, "a (pair, lag)'s words: 66 + 132 cells and two counters");
static_assert(spl::kSlots * kLagLanes * sizeof(unsigned long long) == 51200, "the cells of a workgroup in LDS");
static_assert(3 * (spl::kSlots * kLagLanes + spl::kPairCells) * sizeof(unsigned long long) <= 160 * 1024, "three workgroups fit a CU's 160 KiB");

size_t lagcov_work_bytes(int npairs, int lags)
{
    return sizeof(unsigned long long) * ((size_t)spl::kSlots * (size_t)npairs * (size_t)lags + (size_t)spl::kPairCells * (size_t)npairs);
}

void lagcov_launch_shape(int npairs, int lags, long long terms, int cu_count, long long shape[3])
{
    const int pieces = lagcov_pieces(npairs, lags, terms, cu_count);
    shape[0] = (long long)npairs * lagcov_lag_bands(lags), shape[1] = pieces, shape[2] = (terms + pieces - 1) / pieces;
}

hipError_t launch_lagcov(const double *series, long long width, const int32_t *pairs, int npairs, int lags, void *work, double *out,
                         int cu_count, hipStream_t stream)
{
    unsigned long long *const ws = (unsigned long long *)work;
    unsigned long long *const aws = ws + (size_t)spl::kSlots * (size_t)npairs * (size_t)lags;
    const hipError_t e = hipMemsetAsync(work, 0, lagcov_work_bytes(npairs, lags), stream);
    if (e != hipSuccess) return e;
    const long long terms = spl::terms(width, lags);   // terms + lags - 1 <= width: the accumulate reads no frame past the series
    if (terms > 0) {
        LagPairs p = {};
        for (int k = 0; k < 2 * npairs; k++) p.v[k] = pairs[k];
        long long shape[3];
        lagcov_launch_shape(npairs, lags, terms, cu_count, shape);
        hipLaunchKernelGGL(k_lagcov_accumulate, dim3((unsigned)shape[0], (unsigned)shape[1]), dim3(kLagThreads), 0, stream, series, width, p,
                           lags, terms, shape[2], ws, aws);
    }
    hipLaunchKernelGGL(k_lagcov_finish, dim3((unsigned)((npairs * lags + 63) / 64)), dim3(64), 0, stream, ws, aws, npairs, lags, (int)terms, out);
    return hipSuccess;
}

}  // namespace spk
