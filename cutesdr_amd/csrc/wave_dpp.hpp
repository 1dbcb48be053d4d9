// wave_dpp.hpp -- a wave's scan steps on the DPP network, for the kernels that scan (pc_scan.hpp, noiseblank_kernels.hip).
// A 64-bit __shfl_up is two ds_bpermute -- an LDS-pipe round trip per step; a DPP step is an operand of a vector move.
// The six steps row_shr 1, 2, 4, 8, row_bcast 15 (into rows 1, 3), row_bcast 31 (into rows 2, 3) leave in every lane
// the combination of lanes 0 .. lane, like the six __shfl_up steps (associativity is all they need; a step without a
// source lane reads the identity, which makes the lane guards unnecessary); wave_shr 1 then gives the exclusive value.
#pragma once
#include <hip/hip_runtime.h>

namespace csdr {

// v of the lane the step CTRL reads from, `ident` where the step has no source lane
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long wave_dpp64(unsigned long long v, unsigned long long ident)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)ident, (int)(unsigned)v, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(ident >> 32), (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;
}
#define WAVE_SCAN_STEPS(STEP) STEP(0x111, 0xf) STEP(0x112, 0xf) STEP(0x114, 0xf) STEP(0x118, 0xf) STEP(0x142, 0xa) STEP(0x143, 0xc)
constexpr int WAVE_SHR1 = 0x138;

}  // namespace csdr
