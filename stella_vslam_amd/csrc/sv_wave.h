// Wave-level primitives shared by the ORB, bundle-adjustment and matcher kernels (wave64, gfx9 DPP).
#pragma once
#include <hip/hip_runtime.h>

// one DPP move of a 32-bit or a 64-bit value (the latter as its two halves); lanes the control does not reach read 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int sv_dpp(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double sv_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
// inclusive prefix sum over the 64 lanes, all on the VALU (six __shfl_up would be six LDS-crossbar round trips): scans inside the four rows
// of 16, then the row totals broadcast forward; lane 63 holds the total
template <class T>
__device__ __forceinline__ T sv_wave_inclusive_sum(T v) {
    v += sv_dpp<0x111, 0xF>(v);  // row_shr:1
    v += sv_dpp<0x112, 0xF>(v);  // row_shr:2
    v += sv_dpp<0x114, 0xF>(v);  // row_shr:4
    v += sv_dpp<0x118, 0xF>(v);  // row_shr:8   -> lane 15 of every row holds the row sum
    v += sv_dpp<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
    v += sv_dpp<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}
