// sp_pulse.hip — k_pulse_accumulate, k_pulse_peak_frame and k_pulse_finish (sp_kernel_pulse.h) and their launcher (sp_launch.h): a
// device unit of its own beside sp_burst.hip, whose three launches run in front of these, unchanged.  Host code reaches the kernels
// through the launcher only.
#include <hip/hip_runtime.h>

#include "sp_launch.h"
#include "sp_kernel_pulse.h"

namespace spk {

static_assert(kBandMax == SP_MAX_BANDS, "BurstKeys holds SP_MAX_BANDS thresholds of either kind");

static size_t pulse_bursts(int count, int max_bursts) { return (size_t)(count > 0 ? count : 0) * (size_t)(max_bursts > 0 ? max_bursts : 0); }

size_t pulse_work_bytes(int count, int max_bursts) { return sizeof(unsigned long long) * (spx::kSlots + 1) * pulse_bursts(count, max_bursts); }

hipError_t launch_pulses(const double *series, int count, int width, const uint64_t *hi_key, const uint64_t *lo_key, int max_bursts,
                         const unsigned long long *records, const uint32_t *counts, void *work, double *energy, double *peak,
                         int32_t *peak_at, hipStream_t stream)
{
    if (count <= 0 || width <= 0 || max_bursts <= 0 || !(energy || peak || peak_at)) return hipSuccess;
    BurstKeys keys{};
    for (int b = 0; b < count; b++) {
        keys.hi[b] = hi_key[b];
        keys.lo[b] = lo_key[b];
    }
    const unsigned segments = (unsigned)(((long long)width + kBurstSegment - 1) / kBurstSegment);
    const unsigned long long *const s = (const unsigned long long *)series;
    const unsigned long long *const carries = records + (size_t)count * segments;   // (launch_bursts: the summaries stand in front)
    unsigned long long *const cells = (unsigned long long *)work, *const peak_key = cells + spx::kSlots * pulse_bursts(count, max_bursts);
    const hipError_t e = hipMemsetAsync(work, 0, pulse_work_bytes(count, max_bursts), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(segments, (unsigned)count);
    hipLaunchKernelGGL(k_pulse_accumulate, grid, dim3(kBurstThreads), 0, stream, s, (long long)width, width, keys, carries, max_bursts, cells,
                       peak_key);
    if (peak_at)
        hipLaunchKernelGGL(k_pulse_peak_frame, grid, dim3(kBurstThreads), 0, stream, s, (long long)width, width, keys, carries, max_bursts,
                           (const unsigned long long *)peak_key, peak_at);
    if (energy || peak)
        hipLaunchKernelGGL(k_pulse_finish, dim3((unsigned)((max_bursts + 63) / 64), (unsigned)count), dim3(64), 0, stream, counts, max_bursts,
                           (const unsigned long long *)cells, (const unsigned long long *)peak_key, energy, peak);
    return hipGetLastError();
}

}  // namespace spk
