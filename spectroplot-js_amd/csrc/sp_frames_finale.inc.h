// Finale fragment (k_frames, k_frames_peak): everything behind the group loop, to the end of the kernel body.
// Expects in scope: a, tid, lane, kThreads, smem, s_done, s_red, HALVES, group_frames, drain_x0, gpar, the lambdas side_outputs, drain_rows
// and drain (sp_frames_writeout.inc.h), and what the histogram fragments expect beyond the macros defined here.
    // ---- end of the workgroup's frames: last write-out and side outputs, the workgroup's share of histograms and dBfs range ----------
    const LateArgs la = late_args();
    // requested now, used behind the last barrier: the cell ranges of this thread's histogram outputs and the request's number as
    // workgroup 0 published it
#define SP_LUT_LEN a.lut_len
#define SP_CELLS a.cells
#define SP_REPLY la
#define SP_AFTER_CELLS_READ
#include "sp_frames_hist_ranges.inc.h"
    const unsigned int seen = __hip_atomic_load(la->flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (HALVES && drain_x0 >= 0 && a.rgba) {
        // The workgroup's last write-out overlaps nothing.  The first waves of the SIMDs reach it ~7 us before the second ones (config 2;
        // issue arbitration favours the older wave, s_setprio does not change that - tools/stamps.py) and would wait at the barrier:
        // each set of four waves meets by itself and writes its own half of the group, 64-byte pieces of the image rows, so half of the
        // chip's last stores are under way while the second waves still compute.
        const int half = tid >> 8;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __hip_atomic_fetch_add(&s_done[half], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(&s_done[half], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < 4u) __builtin_amdgcn_s_sleep(2);
        // (non-temporal: left in L2, the 64-byte pieces are written back when the kernel ends, +1.2 us instead of -1.1 us; the first
        // set also taking half of the second set's rows once those are ready: no further gain)
        drain_rows(drain_x0, 0, 1, half * (group_frames / 2), group_frames / 2, half * (kThreads / 2), kThreads / 2, true);
    }
    lds_barrier();
    if (drain_x0 >= 0 && !(HALVES && a.rgba)) drain(drain_x0, 0, 1);
    // ---- the workgroup's share of the request's histograms and dBfs range (worker.js:105-113, 124-125, 140-155) ----------------------
    // No workgroup finishes for the others (that costs the last one three dependent trips to memory, 6 us): every workgroup turns its
    // own merged cells into histogram counts and adds them to the reply itself, with fire-and-forget atomics the launch's end waits
    // for anyway.  Workgroup 0 has zeroed the reply's histograms and set its dBfs range to (0, -200) at the start of the request's
    // first launch and published the request's number behind that (sp_frames_reply_clear.inc.h, sp_frames_publish.inc.h); everybody
    // checks the number before its first add.
    {
        // cells -> prefix sums: every count is a difference of two prefix sums over the cells (sp_host.h Thresholds).  A thread takes
        // kPer consecutive cells, the workgroup scans the 512 partial sums (in each wave with shuffles, the eight wave totals through
        // LDS).  The exchange buffers are idle by now and hold the prefix.  (Counts of one workgroup fit 32 bits, as s_cells does.)
        constexpr int kPer = 3;
        static_assert(kThreads * kPer >= kMaxCells, "every cell needs a thread");
        unsigned int *const s_pre = (unsigned int *)(smem + kOffXch);         // [kThreads * kPer + 1]: s_pre[c] = sum of the cells [0, c)
        unsigned int *const s_part = s_pre + kThreads * kPer + 4;             // [kThreads / 64] wave totals
#include "sp_frames_hist_scan.inc.h"
        if (seen != la->seq) {
            // (never in practice: workgroup 0 - dispatched first: the lowest workgroup number - published the number tens of microseconds
            // ago.  The wait is bounded: ~2 s of polling end in a trap, i.e. a failed launch, instead of a hung device.)
            unsigned polls = 0;
            while (__hip_atomic_load(la->flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != la->seq) {
                __builtin_amdgcn_s_sleep(32);
                if (++polls > (1u << 22)) __builtin_trap();
            }
        }
#include "sp_frames_hist_adds.inc.h"
        // The last group's gauges come behind the adds (two waves, one software log10: ~1 us during which everybody's adds and stores
        // are on their way), and behind them the workgroup's share of the dBfs range.
        if (drain_x0 >= 0) side_outputs(drain_x0, gpar ^ 1);
        lds_barrier();
        double *const out_mm = la->out_minmax;
        if (tid < 2 && out_mm) {
#include "sp_frames_range_atomics.inc.h"
        }
    }
#undef SP_LUT_LEN
#undef SP_CELLS
#undef SP_REPLY
#undef SP_AFTER_CELLS_READ
