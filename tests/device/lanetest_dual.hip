// Lane tests of what a refine round of the BC7 dual-plane search sets up ahead of its pixel loop (csrc/bc7_dual_setup.h): the
// level tables of the two planes against the table they replace, kept here verbatim.  Test code only; nothing here is linked
// into the product.
#include "bc7_dual_setup.h"
#include "lanetest_device.h"

namespace
{
// ---- the level table as it stood before the planes built only what their index reaches: the reference of the comparison ----
__device__ __forceinline__ void levelTableBefore(int e0, int e1, bool threeBit, u32 &tabLo, u32 &tabHi)
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

// One thread per end-point pair (e0, e1) = (t >> 8, t & 255).  The pair sits in one RGB channel and in the alpha channel of a
// configuration whose other channels hold other pairs, and dualLevelTables runs in the three shapes the search has:
// plane 0 = (mode 5) both 2-bit, 1 = (mode 4, index selector 0) alpha 3-bit, 2 = (mode 4, index selector 1) RGB 3-bit.
// `planes` is a kernel argument, so the shape is a scalar the compiler does not know, as in evalDual.
// An input's number: shape << 20 | channel << 16 | t.
__global__ void dualTablesKernel(u32 planes, unsigned long long *__restrict__ result, u32 *__restrict__ two, u32 *__restrict__ threeLo,
                                 u32 *__restrict__ threeHi)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x; // 65 536 threads
    const int e0 = (int)(t >> 8), e1 = (int)(t & 255u);
    unsigned long long mine = 0, first = ~0ull;
    for (u32 shape = 0; shape < 3u; shape++)
    {
        const bool rgb3 = ((planes >> (2 * shape)) & 1u) != 0, alpha3 = ((planes >> (2 * shape + 1)) & 1u) != 0;
        // channel 0: the pair; 1: the pair exchanged; 2: other values; 3 (alpha): the pair
        const int ep[2][4] = {{e0, e1, (e0 * 7 + 3) & 255, e0}, {e1, e0, (e1 * 13 + 5) & 255, e1}};
        u32 lo[4], hi[4];
        dualLevelTables(ep, rgb3, alpha3, lo, hi);
        for (int ch = 0; ch < 4; ch++)
        {
            u32 wantLo, wantHi;
            levelTableBefore(ep[0][ch], ep[1][ch], ch == 3 ? alpha3 : rgb3, wantLo, wantHi);
            if (lo[ch] != wantLo || hi[ch] != wantHi)
            {
                const unsigned long long id = ((unsigned long long)shape << 20) | ((unsigned long long)ch << 16) | t;
                mine++;
                first = first < id ? first : id;
            }
        }
        // the values themselves, for the comparison with numpy: the 2-bit table of the pair (shape 0, alpha) and its 3-bit
        // table (shape 1, alpha)
        if (shape == 0)
            two[t] = lo[3];
        if (shape == 1)
        {
            threeLo[t] = lo[3];
            threeHi[t] = hi[3];
        }
    }
    lanetestReport(result, mine, first);
}
} // namespace

// {mismatches, lowest input} of dualLevelTables against the table before, and the tables of every pair (65 536 words each)
extern "C" hipError_t lanetest_dual_tables(void *d_two, void *d_threeLo, void *d_threeHi, void *d_result, hipStream_t stream)
{
    // shapes 0, 1, 2 as (rgb3, alpha3) bit pairs: (0, 0), (0, 1), (1, 0)
    const u32 planes = 0u | (2u << 2) | (1u << 4);
    hipLaunchKernelGGL(dualTablesKernel, dim3(256), dim3(256), 0, stream, planes, (unsigned long long *)d_result, (u32 *)d_two, (u32 *)d_threeLo,
                       (u32 *)d_threeHi);
    return hipGetLastError();
}
