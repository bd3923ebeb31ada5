// sp_burst.hip — k_burst_summary, k_burst_carry and k_burst_emit (sp_kernel_burst.h) and their launcher (sp_launch.h): a device unit of
// its own beside sp_kernels.hip, whose set of kernels tests/test_isa_checks.py holds to its reference commit's, as sp_band.hip,
// sp_track.hip, sp_occupancy.hip and sp_quantile.hip are.  Host code reaches the kernels through the launcher only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_burst.h"

namespace spk {

static_assert(kBandMax == SP_MAX_BANDS, "BurstKeys holds SP_MAX_BANDS thresholds of either kind");

static unsigned burst_segments(int width) { return (unsigned)(((long long)width + kBurstSegment - 1) / kBurstSegment); }

size_t burst_record_bytes(int count, int width) { return 2 * sizeof(unsigned long long) * (size_t)count * (size_t)burst_segments(width); }

void launch_bursts(const double *series, int count, int width, const uint64_t *hi_key, const uint64_t *lo_key, int max_bursts,
                   unsigned long long *records, uint32_t *counts, int32_t *edges, hipStream_t stream)
{
    if (count <= 0) return;
    BurstKeys keys{};
    for (int b = 0; b < count; b++) {
        keys.hi[b] = hi_key[b];
        keys.lo[b] = lo_key[b];
    }
    const unsigned segments = burst_segments(width);
    const unsigned long long *const s = (const unsigned long long *)series;
    unsigned long long *const summaries = records, *const carries = records + (size_t)count * segments;
    int32_t *const list = max_bursts > 0 ? edges : nullptr;
    const dim3 grid(segments, (unsigned)count);
    if (segments)
        hipLaunchKernelGGL(k_burst_summary, grid, dim3(kBurstThreads), 0, stream, s, (long long)width, width, keys, summaries);
    hipLaunchKernelGGL(k_burst_carry, dim3((unsigned)count), dim3(64), 0, stream, summaries, (int)segments, width, max_bursts, carries, counts,
                       list);
    if (segments && list)
        hipLaunchKernelGGL(k_burst_emit, grid, dim3(kBurstThreads), 0, stream, s, (long long)width, width, keys, carries, max_bursts, list);
}

}  // namespace spk
