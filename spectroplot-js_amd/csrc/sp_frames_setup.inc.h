// Frame-loop fragment (sp_kernel_frames.h explains the fragments): the kernel's shape and LDS layout, the thread's place in them, the
// workgroup's share of the groups.  First in the body of every frame-loop kernel.
// Expects in scope: LOG2N, CH, PFB, a, group_frames, groups.
    constexpr int kThreads = kFrameThreads;   // eight waves, two per SIMD, one workgroup per CU
    constexpr int N = 1 << LOG2N;
    constexpr int T = N / 16;                       // threads per frame
    constexpr int FPB = kThreads / T;               // frames per round
    constexpr bool BLOCK_SYNC = T > 64;
    constexpr int TWMAX = frames_tw_max_stage(N);
    constexpr int NPASS = (LOG2N + 3) / 4;
    constexpr bool PERMLANE_MID = LOG2N == 13;
    constexpr bool STAGED = PFB == 0;   // the generic loaders leave no registers for a whole pass's twiddles: read stage by stage
    // 8-byte samples at n >= 2048: a frame's samples are requested when it starts, not one frame ahead (the prefetch registers of
    // the next frame were what spilled there: cf32, n = 2048: 411 -> 358 us per 32 768 frames); its partner wave covers the latency
    // The L/R split at n >= 2048 likewise (its 16 partner values on top of a frame's 32 spill ~32 registers with the prefetch kept): a
    // spill reload waits for every vector-memory operation issued before it - in-order completion - i.e. for the prefetch itself.
    // Requested at frame start, 12 spilled registers are left and configs 3 / 5 in channel mode take 12 % less time (1.39 -> 1.22 ms,
    // 3.41 -> 2.96 ms).  (The taper from L2 per frame instead of registers: no spills at all, and slower than either.)
    // (8-byte samples with the split at n = 1024: 22 spilled registers -> 0, 90.1 -> 88.0 us at config 2's shape; n = 512: 14 -> 0,
    // 81.6 -> 77.8 us per 2^24 samples; n = 256, 6 spilled registers, is 2 % faster with the prefetch and keeps it)
    constexpr bool LATE_PF = ((PFB == 8 || (CH && PFB != 0)) && LOG2N >= 11) || (CH && PFB == 8 && LOG2N >= 9);

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Layout lay = layout(N, a.lut_len, group_frames);
    double *s_xch = (double *)(smem + kOffXch);
    double2 *s_tw = (double2 *)(smem + lay.off_tw);
    const double *edge_g = (const double *)(smem + lay.off_gedge);
    const double *edge_cb = (const double *)(smem + lay.off_cbedge);
    unsigned long long *s_mm = (unsigned long long *)(smem + lay.off_mm);
    unsigned char *s_tile = smem + lay.off_tile;
    unsigned int *const s_lut = (unsigned int *)(smem + kOffLut);
    unsigned int *const s_cells = (unsigned int *)(smem + kOffCells);
    [[maybe_unused]] unsigned int *s_done = (unsigned int *)(smem + lay.off_done);
    double *s_red = (double *)(smem + lay.off_amp);                           // the workgroup's share of dBfs_min / dBfs_max so far
    double2 *s_amp = (double2 *)(smem + lay.off_amp + 16);                    // [2][group_frames] (I, Q) of sample n/2, by group parity

    // (lds_read_u32 / lds_count address the dynamic LDS block from 0)
    if ((unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    const int tid = threadIdx.x;
    [[maybe_unused]] const int lane = tid & 63;
    const int fs = tid / T;                         // frame slot within a round
    const int tl = tid % T;                         // thread within the frame
    double *xbuf = s_xch + fs * (N + N / 16);
    constexpr bool COUNTER_SYNC = BLOCK_SYNC && T < kThreads;   // a frame's waves are not the whole workgroup (n = 2048, 4096)
    FrameMeet<COUNTER_SYNC, BLOCK_SYNC> meet{
        (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(const __attribute__((address_space(3))) unsigned int *)(s_done + 2 + fs)),
        0u, (unsigned)(T / 64)};
    const int tile_pitch = N + kTilePad;
    const int cmax = a.lut_len - 1;

    // groups are dealt so that workgroups sharing an XCD (blockIdx % 8) own neighbouring groups
    const int xcd = blockIdx.x & 7, lane_in_xcd = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
    const int chunk = (groups + 7) >> 3;
    const int g_end = min(groups, (xcd + 1) * chunk);
