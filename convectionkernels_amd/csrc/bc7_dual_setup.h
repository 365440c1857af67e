// BC7 dual-plane modes 4 / 5: what a refine round sets up ahead of its pixel loop -- the level tables of the two planes.
// Small device functions on their own, so that tests/device/lanetest_dual.hip can sweep them; included by bc7_dual.h.
#pragma once
#include "cvtt_kernel_common.h"

namespace
{
typedef unsigned short v2us __attribute__((ext_vector_type(2)));

// The 4 or 8 reconstructed values of one channel, ((64 - w) * e0 + w * e1 + 32) >> 6 for the BC7 weights w of a 2- or
// 3-bit index (reference IndexSelector.h:90-100), as bytes: tabLo = levels 0..3, tabHi = levels 4..7 (3-bit only).
// Two levels per instruction in packed 16-bit lanes (every intermediate fits 16 bits).
__device__ __forceinline__ void levelTable(int e0, int e1, bool threeBit, u32 &tabLo, u32 &tabHi)
{
    const u32 base = (u32)((e0 << 6) + 32), delta = (u32)(e1 - e0) & 0xffffu;
    const v2us BB = __builtin_bit_cast(v2us, base | (base << 16)), DD = __builtin_bit_cast(v2us, delta | (delta << 16));
    const v2us six = {6, 6};
    // weight pairs: 2-bit {0, 21}, {43, 64}; 3-bit {0, 9}, {18, 27}, {37, 46}, {55, 64}
    const u32 w01 = threeBit ? (0u | (9u << 16)) : (0u | (21u << 16));
    const u32 w23 = threeBit ? (18u | (27u << 16)) : (43u | (64u << 16));
    const v2us r01 = (__builtin_bit_cast(v2us, w01) * DD + BB) >> six;
    const v2us r23 = (__builtin_bit_cast(v2us, w23) * DD + BB) >> six;
    tabLo = __builtin_amdgcn_perm(__builtin_bit_cast(u32, r23), __builtin_bit_cast(u32, r01), 0x06040200u);
    tabHi = 0;
    if (threeBit)
    {
        const v2us r45 = (__builtin_bit_cast(v2us, 37u | (46u << 16)) * DD + BB) >> six;
        const v2us r67 = (__builtin_bit_cast(v2us, 55u | (64u << 16)) * DD + BB) >> six;
        tabHi = __builtin_amdgcn_perm(__builtin_bit_cast(u32, r67), __builtin_bit_cast(u32, r45), 0x06040200u);
    }
}

// The table of a 2-bit index alone.  Levels 0 and 3 are the end points themselves -- ((64 * e0 + 32) >> 6) == e0, and w = 64
// leaves ((64 * e1 + 32) >> 6) == e1 -- so one packed multiply-add gives levels 1 and 2 (weights 21 and 43), and the v_perm_b32
// that packs them takes the end bytes from e0 | e1 << 16: four slow-class instructions for the ten of levelTable, the same
// four bytes (tests/device/lanetest_dual.hip compares the two on all 256^2 pairs).
__device__ __forceinline__ u32 levelTable2(int e0, int e1)
{
    const u32 base = (u32)((e0 << 6) + 32), delta = (u32)(e1 - e0) & 0xffffu;
    const v2us BB = __builtin_bit_cast(v2us, base | (base << 16)), DD = __builtin_bit_cast(v2us, delta | (delta << 16));
    const v2us six = {6, 6};
    const v2us r12 = (__builtin_bit_cast(v2us, 21u | (43u << 16)) * DD + BB) >> six;
    const u32 ends = (u32)e0 | ((u32)e1 << 16);
    return __builtin_amdgcn_perm(__builtin_bit_cast(u32, r12), ends, 0x02060400u);
}

// The tables of the two planes of a configuration.  Which plane has the 3-bit index is wave-uniform (mode 4: alpha at index
// selector 0, RGB at index selector 1; mode 5: neither), so each plane builds only the levels its index can reach, behind a
// scalar branch, instead of all eight per channel with a select afterwards.
__device__ __forceinline__ void dualLevelTables(const int (&ep)[2][4], bool rgbThreeBit, bool alphaThreeBit, u32 (&tabLo)[4], u32 (&tabHi)[4])
{
    if (rgbThreeBit)
    {
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            levelTable(ep[0][ch], ep[1][ch], true, tabLo[ch], tabHi[ch]);
    }
    else
    {
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
        {
            tabLo[ch] = levelTable2(ep[0][ch], ep[1][ch]);
            tabHi[ch] = 0;
        }
    }
    if (alphaThreeBit)
        levelTable(ep[0][3], ep[1][3], true, tabLo[3], tabHi[3]);
    else
    {
        tabLo[3] = levelTable2(ep[0][3], ep[1][3]);
        tabHi[3] = 0;
    }
}
} // namespace
