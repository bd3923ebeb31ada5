// sp_kernel_frames.h — the frame-loop kernel for 64 <= n <= 8192 (gfx950).
//
// lib/worker.js:68-137 per frame (decode, taper, the butterfly graph of lib/fft_nayuki.js:54-96, |X|^2 -> dB -> indices -> RGBA, side
// outputs), built from the parts of sp_frame_parts.h around what bounds it on MI355X.  tools/op_cost.hip (profiles/r02_op_cost.txt): an
// f64 multiply or add costs 4.4-4.7 issue cycles per wave-instruction per SIMD whatever the occupancy, v_permlane32_swap 8, v_log_f32
// 8.5, conversions / floor / fract / compares 4.4, 32-bit integer and f32 multiply-add 2.5; one wave alone reaches half of that, two
// waves reach it.  The reference's unfused butterflies are 800 f64 wave-instructions per 1024-point frame, so the loop is bound by
// VALU issue, not by HBM, LDS or latency, and the design moves work off the VALU or removes it:
//   * first pass (stages 1-4): its eight twiddles cos / sin(2 pi k / 16) are the same doubles for every n >= 16 (the table
//     index k*n/16 is scaled by a power of two before the division by n), so they are literals: no LDS reads, no registers;
//     the butterflies whose twiddle is (1, 0) skip their products when the frame is finite (integer formats always; float
//     frames after one f32 multiply-add per raw word), the ones whose sine is exactly 1 skip two products always;
//   * the re-distribution between passes goes through a padded, wave-private LDS buffer; at n = 512 / 1024 the second one is a
//     register transpose (v_permlane16_swap / v_permlane32_swap: what it costs the VALU the LDS round trip costs the LDS pipe);
//   * input: the raw words of the NEXT frame are requested right after the current frame is decoded (1-, 2-, 3-, 4-, 8-byte samples).
//     One rule follows from the chip completing a wave's vector-memory operations IN ORDER: whatever waits for a younger operation - a
//     reload of a spilled register, a table load - waits for that prefetch too.  So no prefetching variant may spill inside the loop
//     (tests/test_isa_checks.py); the variants that would (8-byte samples at n >= 2048; the L/R split at n >= 2048 and with 8-byte samples
//     from n = 512) request a frame's samples when it starts; and the prologue requests the first frame BEHIND its table loads (n <= 1024);
//   * epilogue: colour index and centi-bel level are floor(a + b*log2(|X|^2)) in f32; a lane is sent to the exact edge tables
//     only if its f32 value lies within a proven error margin of an integer (a few lanes in ten thousand), so the common path has
//     no LDS read and no f64 compare; one histogram atomic per pixel on the merged cell (colour index + level), which the
//     workgroup turns back into the two histograms at its end; one colour byte per pixel into an LDS tile [frame][bin]; frame
//     extremes of |X|^2 by LDS integer atomics on the bit patterns;
//   * after a group of frames the workgroup writes the tile out through the RGBA LUT, in two slices around the passes of the next
//     group's first frame: 16-byte stores, 128-byte row segments in spectrogram layout; in waterfall layout one tile dword per item as
//     four dword stores, 256 contiguous bytes of an image row per wave and store instruction;
//   * n >= 2048 (a frame spans several waves): the waves of a frame meet through an LDS counter, announced early and waited for
//     late where the dataflow allows, instead of the workgroup barrier;
//   * the workgroup's last write-out is split between the first and the second waves of the SIMDs (n = 1024): the first ones
//     finish ~7 us earlier and write their half meanwhile;
//   * the request's side outputs come from this kernel too - one launch per sp_plan_execute: the gauges of a group of frames are
//     evaluated (the reference's software log10, three per frame) by two waves inside the next group, where the first waves of the
//     SIMDs have slack; at its end every workgroup adds its own share of the two histograms and of the dBfs range to the reply with
//     fire-and-forget atomics (workgroup 0 has cleared the reply and published the request's number), so no workgroup waits for
//     another and nothing makes a dependent trip to memory (a last-workgroup ticket costs three: profiles/r04_experiments.txt).
// Measured alternatives (three waves per SIMD, two workgroups per CU, LDS-DMA input, other batch / slice / chain counts) are recorded in
// DESIGN.md section 6.2; the cost-attribution switches and per-wave clock stamps that produced profiles/ live in
// tools/experiments/frames_instrumentation.patch (tools/build_variant.sh applies it), not here.
// The six frame-loop kernels - k_frames (F), k_frames_index (I, sp_kernel_frames_index.h), k_frames_batch (B, ..._batch.h), k_frames_peak
// (P, ..._peak.h), k_frames_traces (T, ..._traces.h), k_frames_power (W, ..._power.h) - are built from fragment files, sp_frames_*.inc.h,
// #included inside the kernel bodies; the loop's order and why it is so is commented there, once.  The inclusion is textual on purpose:
// the compiler sees the tokens it saw when each kernel spelled its loop out, so no kernel's code moves (a shared function, even a local
// alias, moved k_frames' instruction streams; so does a declaration that changes its place - sp_frames_setup.inc.h cannot take the
// four that follow the request in every body).  A fragment's first comment lists the names it expects in scope; an expression that
// differs between the kernels is a macro (SP_X_END, ...) that each kernel defines around the include.  tests/test_isa_checks.py
// compares every instruction stream of the six kernels with a reference build.  Who includes what:
//   * F I        request_body: the whole body of a kernel that renders one request's picture (I defines SP_DRAIN_ROWS_BODY around it);
//   * T W        plain_body: the whole body behind setup of a kernel without a picture, around the kernel's own epilogue per frame
//                (SP_FRAME_TAIL: traces_fold, power_store);
//   * all six    setup, raw_regs (with the HALVES slot mapping), table_loads, table_stores, taper, slot_deal, frame_regs, decode_pf,
//                passes (fft and lr_split, and around them the two write-out slices unless SP_NO_WRITEOUT), directly or through a body;
//   * F I T W    request (the lambda) and next_frame (the next frame, its request, the loaders; F I define SP_TOUCH_AHEAD); load_generic
//                through it, P directly.  B spells both out over its item records, P has request_at and no frame ahead;
//   * F I B P    epilogue_consts, pixels (P defines SP_ABS2); the bodies side_outputs and drain_rows (I: drain_rows_index) inside each
//                kernel's lambdas; hist_ranges, hist_scan, hist_adds and range_atomics (F I P through finale, B in batch_flush);
//   * F I P      the shell of a single request's loop: reply_clear (workgroup 0 clears the reply), publish (the request's number), writeout
//                (the lambdas side_outputs, drain_rows, drain), finale (everything behind the group loop: split last write-out, scan, the
//                bounded poll for the request's number, adds, last side outputs, dBfs range).  B keeps its own lambdas and batch_flush:
//                they read the item record, and its replies are cleared by a kernel queued ahead, so it has no handshake.
// The switches over a format id expand SP_FORMATS_BUT_CF64 (sp_formats.h).
#pragma once

#include <atomic>
#include <cstdio>

#include "sp_frame_parts.h"

namespace spk2 {

using namespace spk;

// cos / sin(2 pi k / 16), k = 0..7, as sphost::twiddles produces them for every n >= 16 (sp_api.hip checks it per plan).
struct Tw16 {
    double c, s;
};
__device__ constexpr Tw16 kTw16[8] = {
    {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.d906bcf328d46p-1, 0x1.87de2a6aea963p-2},
    {0x1.6a09e667f3bcdp-1, 0x1.6a09e667f3bccp-1},
    {0x1.87de2a6aea964p-2, 0x1.d906bcf328d46p-1},
    {0x1.1a62633145c07p-54, 0x1.0000000000000p+0},
    {-0x1.87de2a6aea962p-2, 0x1.d906bcf328d46p-1},
    {-0x1.6a09e667f3bccp-1, 0x1.6a09e667f3bcdp-1},
    {-0x1.d906bcf328d46p-1, 0x1.87de2a6aea965p-2},
};
inline constexpr Tw16 kTw16Host[8] = {
    {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.d906bcf328d46p-1, 0x1.87de2a6aea963p-2},
    {0x1.6a09e667f3bcdp-1, 0x1.6a09e667f3bccp-1},
    {0x1.87de2a6aea964p-2, 0x1.d906bcf328d46p-1},
    {0x1.1a62633145c07p-54, 0x1.0000000000000p+0},
    {-0x1.87de2a6aea962p-2, 0x1.d906bcf328d46p-1},
    {-0x1.6a09e667f3bccp-1, 0x1.6a09e667f3bcdp-1},
    {-0x1.d906bcf328d46p-1, 0x1.87de2a6aea965p-2},
};

// a group's row pieces are written with non-temporal stores from this many frames per group on (4 bytes per frame and row)
#ifndef SP_NT_MIN_GROUP
#define SP_NT_MIN_GROUP 32
#endif

constexpr int kMmSlotsMax = 4;
constexpr int kMaxCells = kLdsMaxLut + SP_CB_HIST_SIZE + 2;   // merged histogram cells (sp_host.h Thresholds)

__host__ __device__ inline constexpr int mm_slots(int n)
{
    return lds_mm_slots(n) < kMmSlotsMax ? lds_mm_slots(n) : kMmSlotsMax;
}

constexpr int kFrameThreads = 512;   // one workgroup per CU: eight waves, two per SIMD

// 16 points per thread, whole frames per workgroup: 64 <= n <= 8192
__host__ __device__ inline bool frames_kernel_supports(int n) { return frame_parts_support(n); }

// n >= 2048: the twiddle tables of stages 1-9 only stay in LDS (stage 10 joins the later ones in L2: two more loads per thread and
// frame), which makes room for a 64 KiB tile: 32 / 16 / 8 frames per group instead of 16 / 8 / 4, i.e. 128 / 64 / 32-byte pieces of
// the image rows and half as many group barriers (config 5 wrote 2.1 x its image with 16-byte pieces; config 3: -0.7 %, cf32 at
// n = 2048: -5 %, config 5: -5 %)
__host__ __device__ inline constexpr int frames_tw_max_stage(int n) { return n >= 2048 ? 9 : kLdsTwMaxStage; }
__host__ __device__ inline constexpr int frames_tw_entries(int n) { return n < (1 << frames_tw_max_stage(n)) ? n : (1 << frames_tw_max_stage(n)); }

// frames per output group (tile height): a multiple of the frames per round and of 4 (the write-out handles frame quads)
__host__ __device__ inline int group_frames_for(int n, int want)
{
    const int fpb = kFrameThreads * 16 / n;
    int unit = fpb;
    while (unit % 4) unit *= 2;          // lcm(fpb, 4) for fpb in {1, 2, 3, 6, 12, ...}
    int cap = (n >= 2048 ? 65536 : 32768) / n;
    if (cap > want) cap = want;
    int f = cap / unit * unit;
    if (f < unit) f = unit;
    return f;
}

// n <= 1024: a group's side outputs are evaluated behind the SECOND barrier of the following group's first frame, which takes a second
// set of frame-extreme slots (n >= 2048 has no LDS left for one: they are evaluated behind the first barrier there)
__host__ __device__ inline constexpr bool late_side_outputs(int n) { return n <= 1024; }

// The RGBA LUT and the merged histogram cells sit at FIXED LDS addresses in front of everything whose size depends on the request, so
// that a pixel's LUT read and its histogram atomic are `ds_* vaddr offset:imm` with vaddr = index * 4 alone: one VALU instruction per
// pixel for either address (v_lshlrev_b32_sdwa of a tile byte; v_add_lshl_u32 of colour index + level) instead of two.
constexpr int kOffLut = 0;                                        // u32[kLdsMaxLut]
constexpr int kOffCells = kOffLut + kLdsMaxLut * 4;               // u32[kMaxCells]: word c counts the pixels with colour index + level == c
constexpr int kOffXch = (kOffCells + kMaxCells * 4 + 15) & ~15;   // exchange buffers, then the rest of Layout

struct Layout {
    int off_tw, off_gedge, off_cbedge, off_mm, off_tile, off_done, off_amp, off_win, total;
};

__host__ __device__ inline Layout layout(int n, int lut_len, int group_frames)
{
    Layout l;
    const int fpb = kFrameThreads * 16 / n;
    int o = kOffXch + fpb * (n + n / 16) * 8;                    // exchange buffers
    l.off_tw = o;     o += frames_tw_entries(n) * 16;
    l.off_gedge = o;  o += lut_len * 8;                          // exact edge tables (read by the few lanes the f32 test sends there)
    l.off_cbedge = o; o += (SP_CB_HIST_SIZE + 1) * 8;
    o = (o + 15) & ~15;
    l.off_mm = o;     o += (late_side_outputs(n) ? 2 : 1) * group_frames * mm_slots(n) * 2 * 8;   // frame extremes (n <= 1024: by group parity)
    l.off_tile = o;   o += (group_frames * (n + kTilePad) + 15) & ~15;
    l.off_done = o;   o += 32;                                   // arrival counters: the two wave sets (last write-out), the frames' waves; [7]: "last workgroup"
    o = (o + 15) & ~15;
    l.off_amp = o;    o += 16 + 2 * group_frames * 16;           // the workgroup's extreme |X|^2 so far; raw centre samples of two groups' frames
    l.off_win = o;    o += lds_win_in_lds(n) ? n * 8 : 0;
    l.total = (o + 15) & ~15;
    return l;
}

// v_min_f64 / v_max_f64 as single instructions: fmin() / fmax() first quiet a possible signalling NaN in each operand with a
// v_max_f64 x, x, x of its own, three instructions per call.  The hardware minimum / maximum already ignores a (quiet) NaN
// operand, which is all the frame extremes need (worker.js:102-103: comparisons with NaN are false).
__device__ inline double min_raw(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ inline double max_raw(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Fire-and-forget LDS minimum / maximum of doubles (no NaN operands here).  As instructions: the compiler's atomic optimiser turns
// an atomic with a wave-uniform address into a loop over the active lanes, ~10 instructions per lane; the LDS serialises the lanes itself.
__device__ inline void lds_min_f64(double *p, double v)
{
    asm volatile("ds_min_f64 %0, %1" ::"v"((unsigned)(size_t)(__attribute__((address_space(3))) double *)p), "v"(v) : "memory");
}
__device__ inline void lds_max_f64(double *p, double v)
{
    asm volatile("ds_max_f64 %0, %1" ::"v"((unsigned)(size_t)(__attribute__((address_space(3))) double *)p), "v"(v) : "memory");
}

// Inclusive prefix sum over the 64 lanes of a wave in the VALU: row shifts, then the two row broadcasts of the GFX9 family (a shuffle
// scan is six dependent trips through the LDS crossbar).
__device__ inline unsigned wave_scan_u32(unsigned x)
{
#define SP_DPP_ADD(ctrl, rows) x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, rows, 0xf, false);
    SP_DPP_ADD(0x111, 0xf)   // row_shr:1
    SP_DPP_ADD(0x112, 0xf)   // row_shr:2
    SP_DPP_ADD(0x114, 0xf)   // row_shr:4
    SP_DPP_ADD(0x118, 0xf)   // row_shr:8
    SP_DPP_ADD(0x142, 0xa)   // row_bcast:15 -> rows 1, 3
    SP_DPP_ADD(0x143, 0xc)   // row_bcast:31 -> rows 2, 3
#undef SP_DPP_ADD
    return x;
}

// 16-byte non-temporal store (dst is 16-byte aligned)
__device__ inline void store_nt(uint8_t *dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {a, b, c, d};
    __builtin_nontemporal_store(v, (u32x4 *)dst);
}

// 16-byte store at a wave-uniform base + a 32-bit lane offset: `global_store_dwordx4 voff, data, s[base]`.  From `base + off` the
// compiler builds the 64-bit address in the VALU (a v_mov of the zero high half and a v_lshl_add_u64 per store).
__device__ inline void store16_at(uint8_t *base, unsigned off, uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool nt)
{
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {a, b, c, d};
    if (nt) asm volatile("global_store_dwordx4 %0, %1, %2 nt" ::"v"(off), "v"(v), "s"(base) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, %2" ::"v"(off), "v"(v), "s"(base) : "memory");
}

// LDS accesses at a compile-time offset plus a byte offset held in a VGPR, through a pointer made from the integer (the dynamic LDS
// block starts at address 0: k_frames has no static LDS and checks it once): `ds_* vaddr offset:imm`.  Going through `smem + ...`
// instead leaves a `v_add_u32 v, 0, v` per access behind - the block's address is only replaced by its value after the last folding pass.
typedef __attribute__((address_space(3))) uint32_t *LdsU32;
__device__ inline uint32_t lds_read_u32(int fixed_off, unsigned var_off) { return *(LdsU32)(uintptr_t)(unsigned)(fixed_off + var_off); }
__device__ inline void lds_count(int fixed_off, unsigned var_off)
{
    __hip_atomic_fetch_add((LdsU32)(uintptr_t)(unsigned)(fixed_off + var_off), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// 4 * byte J of a dword in ONE instruction (sub-dword addressing): the LDS byte offset of a tile byte's LUT entry.
template <int J>
__device__ inline unsigned byte_times4(unsigned w)
{
    unsigned r;
    if constexpr (J == 0) asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(w));
    else if constexpr (J == 1) asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(w));
    else if constexpr (J == 2) asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(w));
    else asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(w));
    return r;
}

// Does any of the raw f32 words (lo[e], hi[e]: the two halves of one 64-bit load) hold an infinity or a NaN?  x*0 is NaN exactly for
// those; v_pk_fma_f32 takes a sample's two words at once.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The launch arguments as they lie in the kernel-argument segment (FrameArgs is k_frames' first parameter), behind an opaque copy of
// the segment pointer: fields read through it are fetched (s_load) where they are used - the side outputs once per group, the
// request's end - instead of sitting in SGPRs from the kernel's first instruction on (the compiler loads every field of a by-value
// argument it can see at the entry; the two dozen that only the side outputs need cost as many spilled SGPRs in the frame loop).
typedef const __attribute__((address_space(4))) FrameArgs *LateArgs;
__device__ inline LateArgs late_args()
{
    LateArgs p = (LateArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// First register pass: stages 1-4 inside window [0, 4) with literal twiddles.
template <bool TRIV>
__device__ inline void fft_pass1(double (&re)[16], double (&im)[16])
{
#pragma unroll
    for (int s = 1; s <= 4; s++) {
        const int u = s - 1;
#pragma unroll
        for (int e0 = 0; e0 < 16; e0++) {
            if (e0 & (1 << u)) continue;
            const int e1 = e0 | (1 << u);
            const int k = (e0 & ((1 << u) - 1)) << (4 - s);     // fft_nayuki.js:76-78: table index j * n / size, in units of n / 16
            const double c = kTw16[k].c, sn = kTw16[k].s;
            const double rl = re[e1], il = im[e1];
            double tpre, tpim;                                   // fft_nayuki.js:80-81
            if (TRIV && k == 0) {
                // (1, 0): x*1 + y*0 == x bit for bit for finite x, y (only the sign of a zero can differ; nothing depends on it)
                tpre = rl;
                tpim = il;
            } else if (k == 4) {
                // sine exactly 1: y*1 == y for every y, NaN and infinities included
                tpre = rl * c + il;
                tpim = il * c - rl;
            } else {
                tpre = rl * c + il * sn;
                tpim = il * c - rl * sn;
            }
            const double rj = re[e0], ij = im[e0];
            re[e1] = rj - tpre;
            im[e1] = ij - tpim;
            re[e0] = rj + tpre;
            im[e0] = ij + tpim;
        }
    }
}

template <int NHI>
__device__ inline bool raw_f32_nonfinite(const uint32_t (&lo)[16], const uint32_t (&hi)[NHI])
{
    static_assert(NHI == 16, "8-byte samples: two f32 words each");
    unsigned long long s = 0ull;
    const unsigned long long zero = 0ull;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const unsigned long long w = ((unsigned long long)hi[e] << 32) | lo[e];   // the register pair the 64-bit load filled
        asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(s) : "v"(w), "v"(zero));
    }
    const float s0 = __uint_as_float((uint32_t)s), s1 = __uint_as_float((uint32_t)(s >> 32));
    return __ballot(s0 != s0 || s1 != s1) != 0ull;
}


// The waves that share a frame (n = 2048: two, n = 4096: four) meet through an LDS counter instead of the workgroup barrier, which
// held every frame of a round to the pace of the slowest wave and kept all waves in the same phase (all in the VALU, then all in the
// LDS).  Every LDS operation a wave has issued is ahead of its increment in the LDS queue (a wave's LDS operations execute in
// order), so "my writes are visible" and "my reads are done" both hold once the partners see the count.
template <bool COUNTER, bool BLOCK_SYNC>
struct FrameMeet {
    unsigned addr;     // LDS byte address of the frame's counter (wave-uniform)
    unsigned target;   // the count once every wave of the frame has arrived the next time
    unsigned step;     // waves per frame
    // One asm block each (a C loop around an atomic splits the kernel's big basic blocks and costs the register allocator 60+ spilled
    // VGPRs).  arrive(): lane 0 adds one.  wait(): the wave polls until every wave of the frame has arrived as often as itself.
    // A wave alternates arrive and wait strictly, so no wave is ever two arrivals ahead and the count cannot be reached early.
    __device__ inline void arrive()
    {
        if constexpr (COUNTER) {
            unsigned long long save;
            unsigned a_v, one_v;
            asm volatile("v_mov_b32 %[a_v], %[addr]\n\t"
                         "v_mov_b32 %[one_v], 1\n\t"
                         "s_mov_b64 %[save], exec\n\t"
                         "s_mov_b64 exec, 1\n\t"
                         "ds_add_u32 %[a_v], %[one_v]\n\t"
                         "s_mov_b64 exec, %[save]"
                         : [save] "=&s"(save), [a_v] "=&v"(a_v), [one_v] "=&v"(one_v)
                         : [addr] "s"(addr)
                         : "memory");
        }
    }
    __device__ inline void wait()
    {
        if constexpr (COUNTER) {
            target = (unsigned)__builtin_amdgcn_readfirstlane((int)(target + step));   // wave-uniform, kept in an SGPR
            unsigned a_v, got_v, got_s;
            asm volatile("v_mov_b32 %[a_v], %[addr]\n"
                         "L_sp_meet_%=:\n\t"
                         "ds_read_b32 %[got_v], %[a_v]\n\t"
                         "s_waitcnt lgkmcnt(0)\n\t"
                         "v_readfirstlane_b32 %[got_s], %[got_v]\n\t"
                         "s_sub_i32 %[got_s], %[got_s], %[target]\n\t"
                         "s_cmp_lt_i32 %[got_s], 0\n\t"
                         "s_cbranch_scc1 L_sp_meet_%="
                         : [a_v] "=&v"(a_v), [got_v] "=&v"(got_v), [got_s] "=&s"(got_s)
                         : [addr] "s"(addr), [target] "s"(target)
                         : "memory", "scc");
        } else {
            spk::frame_sync<BLOCK_SYNC>();
        }
    }
    __device__ inline void operator()()
    {
        arrive();
        wait();
    }
};

template <int LOG2N, bool CH, int PFB>
__global__ __launch_bounds__(kFrameThreads, 1) void k_frames(const FrameArgs a, const int format, const double2 *__restrict__ stage_tw,
                                                       const int group_frames, const int groups)
{
#include "sp_frames_request_body.inc.h"
}

// The launch rules of the frame-loop kernels (sp_api.hip's batch plan follows them too).
// Frames per group for a launch over total_frames frames: 32, or fewer while that leaves less than two groups per CU.
inline int frames_group_frames(int n, int64_t total_frames, int cu_count)
{
    int want = 32;
    while (want > 4 && (total_frames + want - 1) / want < 2 * (int64_t)cu_count) want >>= 1;
    return group_frames_for(n, want);
}

// Workgroups: at most one per CU, a multiple of the eight XCDs.
inline int frames_grid(int groups, int cu_count)
{
    const int g = groups < cu_count ? groups : cu_count;
    return (g + 7) & ~7;
}

// The prefetching loader of a capture (its sample width), or 0 for the generic loaders: every frame must lie inside the capture, and
// with 3-byte samples the last frame must start past sample 0.
inline int frames_prefetch_width(int sample_width, bool in_bounds, double stride, int width)
{
    const int p = in_bounds && (sample_width <= 4 || sample_width == 8) ? sample_width : 0;
    return p == 3 && !(width >= 2 && frame_start(stride, width - 1) >= 1) ? 0 : p;
}

// The shape of one launch: frames per group, groups, workgroups, dynamic LDS bytes.
struct FramesLaunch {
    int gf, groups, grid, lds_bytes;
};

// The one launch rule.  `count` frames (k_frames) or columns (k_frames_peak) are dealt into groups by frames_group_frames; with
// gf_fixed > 0 (k_frames_batch) the caller has dealt its items into `count` groups of gf_fixed frames already.  Returns SP_OK and the
// launch's shape, or SP_ERR_UNSUPPORTED.
inline int frames_launch_rule(int n, int lut_len, int64_t count, int cu_count, int gf_fixed, FramesLaunch &fl)
{
    if (!frames_kernel_supports(n) || lut_len > kLdsMaxLut || lut_len < 2) return SP_ERR_UNSUPPORTED;
    fl.gf = gf_fixed > 0 ? gf_fixed : frames_group_frames(n, count, cu_count);
    if (fl.gf & (fl.gf - 1)) return SP_ERR_UNSUPPORTED;   // (the write-out splits item numbers with shifts; every n in range gives a power of two)
    fl.groups = (int)(gf_fixed > 0 ? count : (count + fl.gf - 1) / fl.gf);
    fl.lds_bytes = layout(n, lut_len, fl.gf).total;
    if (fl.lds_bytes > 160 * 1024) return SP_ERR_UNSUPPORTED;
    fl.grid = frames_grid(fl.groups, cu_count);
    return SP_OK;
}

// One launch of a variant of a frame-loop kernel, behind its per-device opt-in to the full LDS (function attributes belong to the
// device's code object).  (Contexts of several devices render on different threads: the flags are atomic, and setting the attribute
// twice is harmless.)
template <auto Kernel, typename... Args>
inline int launch_full_lds(int grid, int lds_bytes, int device, hipStream_t stream, const Args &...args)
{
    static std::atomic<bool> attr_set[kMaxDevices];
    if (device < 0 || device >= kMaxDevices || !attr_set[device].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return SP_ERR_HIP;
        if (device >= 0 && device < kMaxDevices) attr_set[device].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(kFrameThreads), (size_t)lds_bytes, stream, args...);
    return SP_OK;
}

// Per-n launchers, one translation unit each (sp_inst_frames.hip is compiled once per kernel family and LOG2N):
// NAME<L>(a, format, stage_tw, fl, prefetch, device, stream, <what the kernel takes behind `groups`>).
// SP_DECLARE_LAUNCH_N(NAME, SIZES, extra parameter types...) declares NAME and its specialisation for every L of SIZES.
#define SP_LAUNCH_N_PARAMS \
    const FrameArgs &a, int format, const double2 *stage_tw, const FramesLaunch &fl, int prefetch, int device, hipStream_t stream
#define SP_SIZES_6_10(X, ...) X(6, __VA_ARGS__) X(7, __VA_ARGS__) X(8, __VA_ARGS__) X(9, __VA_ARGS__) X(10, __VA_ARGS__)
#define SP_SIZES_6_13(X, ...) SP_SIZES_6_10(X, __VA_ARGS__) X(11, __VA_ARGS__) X(12, __VA_ARGS__) X(13, __VA_ARGS__)
#define SP_DECLARE_LAUNCH_N_AT(L, NAME, ...) \
    template <>                              \
    int NAME<L>(SP_LAUNCH_N_PARAMS, ##__VA_ARGS__);
#define SP_DECLARE_LAUNCH_N(NAME, SIZES, ...)       \
    template <int L>                                \
    int NAME(SP_LAUNCH_N_PARAMS, ##__VA_ARGS__);    \
    SIZES(SP_DECLARE_LAUNCH_N_AT, NAME, ##__VA_ARGS__)

// The body of a per-n launcher: SP_LAUNCH_VARIANT(KERNEL, extra arguments...) launches KERNEL<L, a.channel_mode, prefetch> and returns.
// SP_LAUNCH_VARIANT_IF(BUILT, KERNEL, extra arguments...) does so for the variants that the predicate BUILT(n, channel_mode, prefetch)
// keeps and returns SP_ERR_UNSUPPORTED for the others, which are not compiled either: the generic lambda is a template, and a
// template's discarded branch is not instantiated.  Expects in scope: L and the parameters of SP_LAUNCH_N_PARAMS.
template <bool C, int P>
struct Variant {
    static constexpr bool c = C;
    static constexpr int p = P;
};
constexpr bool frames_variant_built(int, bool, int) { return true; }
#define SP_LAUNCH_VARIANT_C(C)                      \
    switch (prefetch) {                             \
    case 8: return launch_cp(Variant<C, 8>{});      \
    case 4: return launch_cp(Variant<C, 4>{});      \
    case 3: return launch_cp(Variant<C, 3>{});      \
    case 2: return launch_cp(Variant<C, 2>{});      \
    case 1: return launch_cp(Variant<C, 1>{});      \
    default: return launch_cp(Variant<C, 0>{});     \
    }
#define SP_LAUNCH_VARIANT_IF(BUILT, KERNEL, ...)                                                                                       \
    auto launch_cp = [&](auto v) -> int {                                                                                              \
        using V = decltype(v);                                                                                                         \
        if constexpr (BUILT(1 << L, V::c, V::p))                                                                                       \
            return launch_full_lds<KERNEL<L, V::c, V::p>>(fl.grid, fl.lds_bytes, device, stream, a, format, stage_tw, fl.gf, fl.groups, \
                                                          ##__VA_ARGS__);                                                              \
        else return SP_ERR_UNSUPPORTED;                                                                                                \
    };                                                                                                                                 \
    if (a.channel_mode) { SP_LAUNCH_VARIANT_C(true) } else { SP_LAUNCH_VARIANT_C(false) }
#define SP_LAUNCH_VARIANT(KERNEL, ...) SP_LAUNCH_VARIANT_IF(frames_variant_built, KERNEL, ##__VA_ARGS__)

// The end of a host-side launch: SP_LAUNCH_LEVELS(SIZES, NAME, extra arguments...) returns NAME<a.levels>(...) for the sizes of SIZES,
// SP_ERR_UNSUPPORTED for any other.  Expects in scope: prefetch, fl and the launch's a, format, stage_tw, device, stream.
#define SP_LAUNCH_LEVELS_AT(L, NAME, ...) \
    case L: return NAME<L>(a, format, stage_tw, fl, prefetch, device, stream, ##__VA_ARGS__);
#define SP_LAUNCH_LEVELS(SIZES, NAME, ...)              \
    switch (a.levels) {                                 \
        SIZES(SP_LAUNCH_LEVELS_AT, NAME, ##__VA_ARGS__) \
    default: return SP_ERR_UNSUPPORTED;                 \
    }

SP_DECLARE_LAUNCH_N(launch_frames_n, SP_SIZES_6_13)

#ifdef SP_INST_FRAMES_LOG2N
template <>
int launch_frames_n<SP_INST_FRAMES_LOG2N>(SP_LAUNCH_N_PARAMS)
{
    constexpr int L = SP_INST_FRAMES_LOG2N;
    SP_LAUNCH_VARIANT(k_frames)
}
#endif

// Host-side launch.  Returns SP_OK or SP_ERR_UNSUPPORTED.
inline int launch_frames(const FrameArgs &a, int format, const double2 *stage_tw, int cu_count, int device, hipStream_t stream)
{
    const int prefetch = frames_prefetch_width(a.sample_width, a.in_bounds, a.stride, a.width);
    FramesLaunch fl;
    if (frames_launch_rule(a.n, a.lut_len, a.x_end - a.frame0, cu_count, 0, fl)) return SP_ERR_UNSUPPORTED;
    SP_LAUNCH_LEVELS(SP_SIZES_6_13, launch_frames_n)
}

}  // namespace spk2
