// sp_wave_sum.h — the exact sum of one 32-bit word per lane over a wave's 64 lanes, in the VALU: what the folds in front of the LDS and
// global atomics share (band_fold of sp_kernel_band.h, pulse_wave_sum of sp_kernel_pulse.h).
#pragma once

#include <hip/hip_runtime.h>

namespace spk {

// wave_row_sums: lane 15 of every row of 16 lanes gets the row's sum (the other lanes a prefix of it), by four row_shr DPP adds.
// wave_rows_total: the sum of the four row sums, one readlane each.  EVERY lane of the wave must be here: the DPP adds read their
// neighbours.  The adds are 32-bit and nothing looks after a carry: the caller bounds the addends so that 16 of them stay below 2^32
// (the total of the four rows is 64-bit).
__device__ inline uint32_t wave_row_sums(uint32_t x)
{
#define SP_DPP_ADD(ctrl) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, 0xf, 0xf, false);
    SP_DPP_ADD(0x111)   // row_shr:1
    SP_DPP_ADD(0x112)   // row_shr:2
    SP_DPP_ADD(0x114)   // row_shr:4
    SP_DPP_ADD(0x118)   // row_shr:8
#undef SP_DPP_ADD
    return x;
}
template <typename T = unsigned long long>   // (uint32_t where the caller knows that the total is one word: the adds are 32-bit then)
__device__ inline T wave_rows_total(uint32_t x)
{
    return (T)(uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

}  // namespace spk
