// Wave primitives of the ETC2 colour kernel: the wave-level fence, small exact divisions, uniform values moved to scalar
// registers, lane reads, the xor butterflies and the wave-wide argmin.  Part of etc2_kernel.hip (one translation unit).
#pragma once
#include <type_traits>

namespace
{
#define WAVE_SYNC()                                          \
    do                                                       \
    {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                     \
    } while (0)

// v_min_f32 of two values known not to be NaN (sums of squares read back from LDS): __builtin_fminf on loaded values makes
// the compiler canonicalise both operands first (two v_max_f32 per minimum)
__device__ __forceinline__ float minLoaded(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ int udivSmall(int n, int d)
{
    // exact n / d for 0 <= n < 2^16, 0 < d < 2^12 (integer divisions of ETC.cpp:446, 546, 717).  v_rcp_f32 (1 ulp) is enough:
    // the product is within 0.02 of n / d, so the truncated value is off by at most one, which the two corrections undo
    // (__frcp_rn is a full IEEE division sequence under -fhip-fp32-correctly-rounded-divide-sqrt: twenty instructions)
    int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
    const int r = n - q * d;
    if (r < 0) q--;
    if (r >= d) q++;
    return q;
}

// ceil(2^20 / d) for 1 <= d <= 128 (one float division with the two possible corrections, per EAC candidate)
__device__ __forceinline__ int udivSmall20(int d)
{
    int q = (int)(1048576.0f * __builtin_amdgcn_rcpf((float)d));
    int r = 1048576 - q * d;
    if (r < 0) { q--; r += d; }
    if (r >= d) { q++; r -= d; }
    return r == 0 ? q : q + 1;
}

// A value that is the same in every lane (a wave-wide winner, a best-so-far) moved to a scalar register: the compiler cannot
// see the uniformity through shuffles and LDS reads and would keep one copy per lane alive across the search phases.
__device__ __forceinline__ u32 uniU(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int uniI(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniF(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// the value lane `lane` holds, `lane` the same in every lane: v_readlane_b32 (a scalar result) instead of a ds_bpermute_b32
__device__ __forceinline__ int laneI(int v, int lane) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane)); }
__device__ __forceinline__ float laneF(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), __builtin_amdgcn_readfirstlane(lane))); }
// The value of lane (l ^ M), M a power of two: ds_swizzle_b32 in bit mode inside the 32-lane halves (no address register, a
// third of the LDS-crossbar time of ds_bpermute_b32), ds_bpermute_b32 across them.  __shfl_xor computes its lane index with the
// wave-size arithmetic of amd_warp_functions.h, whose common subexpression the compiler kept alive -- and spilled -- through the
// whole kernel.
template <int M>
__device__ __forceinline__ int xorLaneI(int v)
{
    if (M < 32)
        return __builtin_amdgcn_ds_swizzle(v, (M << 10) | 0x1f);
    return __builtin_amdgcn_ds_bpermute((int)((threadIdx.x ^ 32u) << 2), v);
}
template <int M>
__device__ __forceinline__ float xorLaneF(float v) { return __int_as_float(xorLaneI<M>(__float_as_int(v))); }

// f(M) for every xor step M of the list, in order: the butterflies (minimum, OR, argmin ...) over the lanes that differ in
// those bits.  M arrives as a std::integral_constant: f hands M.value on to xorLaneI / xorLaneF.
template <int... M, typename F>
__device__ __forceinline__ void butterfly(F f)
{
    (f(std::integral_constant<int, M>{}), ...);
}

// wave-wide argmin of (err, id); ties -> lowest id.  All lanes receive the winner (as scalars: what is derived from it is scalar
// arithmetic).  The errors are sums of squares or FLT_MAX -- no NaN, no -0 -- so the lexicographic minimum of (err, id) is the
// minimum of the errors (six ds_swizzle + v_min_f32) followed by the lowest id among the lanes that hold it: nearly always ONE
// lane (a ballot, s_ff1, v_readlane), otherwise a second reduction over the ids.  (Round 5: the pair-at-a-time form -- two
// swizzles, two compares, two selects per step -- was a third of the pair walk's instructions.)
// An error that IS NaN (infinite weights: 0 * inf) would leave the lanes with different minima -- minLoaded keeps its second
// operand on an unordered compare -- and the id without a holder: such errors count as FLT_MAX, so the id returned is always
// one of the candidates (one v_cmp_u_f32 and a scalar branch in the common path).
__device__ __forceinline__ void waveArgmin(float &err, int &id)
{
    if (__ballot(err != err) != 0)
        err = (err == err) ? err : FLT_MAX;
    float m = err;
    m = minLoaded(m, xorLaneF<1>(m));
    m = minLoaded(m, xorLaneF<2>(m));
    m = minLoaded(m, xorLaneF<4>(m));
    m = minLoaded(m, xorLaneF<8>(m));
    m = minLoaded(m, xorLaneF<16>(m));
    m = minLoaded(m, xorLaneF<32>(m));
    const bool mine = err == m;
    const u64 holders = __ballot(mine);
    int best;
    if (__popcll(holders) == 1)
        best = __builtin_amdgcn_readlane(id, __ffsll((long long)holders) - 1);
    else
    {
        int c = mine ? id : 0x7fffffff;
        butterfly<1, 2, 4, 8, 16, 32>([&](auto m) { const int o = xorLaneI<m.value>(c); c = o < c ? o : c; });
        best = __builtin_amdgcn_readfirstlane(c);
    }
    err = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
    id = best;
}
} // namespace
