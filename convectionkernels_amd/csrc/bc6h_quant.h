// BC6H end-point arithmetic: quantise / unquantise, TwosCLHalfToFloat, the 24-bit interpolant reconstruction, and the quad /
// group lane helpers of cvttmi_bc6h_kernel.  Part of bc6h_kernel.hip (one translation unit), included behind its knobs.
#pragma once

namespace
{
// ceil(n / 31), exact for 0 <= n < 8 367 148: one v_mul_hi_u32.  2216757579 = (2^36 + 8213) / 31 (NOT ceil(2^36 / 31) = 2216757315):
// x * 2216757579 / 2^36 = x / 31 + x * 8213 / (31 * 2^36), and x / 31 lies at least 1 / 31 below the next integer, so the
// floor is that of x / 31 while x * 8213 < 2^36 where x = n + 30 = 30 (mod 31); n = 8 367 148 is the first to come out one too
// high (swept on the device; the callers pass at most 31743 * 64)
__device__ __forceinline__ int ceilDiv31(int n)
{
    return (int)(__umulhi((u32)(n + 30), 2216757579u) >> 4);
}

// QuantizeSingleEndpointElementUnsigned, BC67.cpp:2441-2445.  The reference divides elem * 64 by 31 in binary32 rounded
// up (RoundUpForScope, BC67.cpp:2556), subtracts 32768, takes the ceiling and re-biases.  For every elem the colour-space
// clamp lets through (0 ... 31743) that is the integer ceil(elem * 64 / 31): the quotient rounded up never passes the next
// integer (integers below 2^24 are representable), and its distance from the integer below is at least 1/31, far above
// half an ulp of the difference -- checked exhaustively against the float sequence by tools/check_bc6h_quantize.py.
__device__ __forceinline__ int quantizeUnsigned(int elem, int precision)
{
    return ceilDiv31(elem * 64) >> (16 - precision);
}

// QuantizeSingleEndpointElementSigned, BC67.cpp:2425-2439: ceil(|elem| * 32 / 31), by the same argument (|elem| <= 31743)
__device__ __forceinline__ int quantizeSigned(int elem, int precision)
{
    const bool neg = elem < 0;
    int a = neg ? -elem : elem;
    int i = ceilDiv31(a * 32);
    i = i > 32767 ? 32767 : i;
    a = (int)(((u32)i & 0xffffu) >> (16 - precision));
    return neg ? -a : a;
}

// Unquantize*, BC67.cpp:2447-2501: returns the interpolation endpoint, `finished` = colour-space value
__device__ __forceinline__ int unquantizeUnsigned(int comp, int precision, int &finished)
{
    u32 unq = (u32)comp & 0xffffu;
    if (precision < 15)
    {
        unq = (((u32)comp << (16 - precision)) + (0x8000u >> precision)) & 0xffffu;
        if (comp == 0) unq = 0;
        if (((1 << precision) - 2) < comp) unq = 0xffffu;
    }
    finished = (int)((unq * 31u) >> 6);
    return (int)unq;
}

__device__ __forceinline__ int unquantizeSigned(int comp, int precision, int &finished)
{
    const bool neg = comp < 0;
    const int absComp = neg ? -comp : comp;
    int unq, absUnq;
    if (precision >= 16)
    {
        unq = comp;
        absUnq = absComp;
    }
    else
    {
        absUnq = (int)(short)(unsigned short)((absComp << (16 - precision)) + (0x4000 >> (precision - 1)));
        if (comp == 0) absUnq = 0;
        if (((1 << (precision - 1)) - 2) < comp) absUnq = 0x7fff;
        unq = neg ? -absUnq : absUnq;
    }
    int funq = (int)((((u32)absUnq & 0xffffu) * 31u) >> 5);
    funq = funq > 32767 ? 32767 : funq;
    finished = (int)(short)(neg ? -funq : funq);
    return (int)(short)unq;
}

// channel ch of both end points of a subset
template <bool SIGNED>
__device__ __forceinline__ void unquantizeBoth(int q0, int q1, int precision, int (&unq)[2][3], int (&fin)[2][3], int ch)
{
    unq[0][ch] = SIGNED ? unquantizeSigned(q0, precision, fin[0][ch]) : unquantizeUnsigned(q0, precision, fin[0][ch]);
    unq[1][ch] = SIGNED ? unquantizeSigned(q1, precision, fin[1][ch]) : unquantizeUnsigned(q1, precision, fin[1][ch]);
}

// TwosCLHalfToFloat, ParallelMath.h:1012-1041 -- literal bit manipulation (needed for the
// signed format, whose negative 2CL pixel values are not valid half patterns)
__device__ __forceinline__ float twosCLHalfToFloatBits(int v16)
{
    const u32 v = (u32)v16 & 0xffffu;
    const u32 signBits = v & 0x8000u;
    const u32 mantissa = v & 0x03ffu;
    u32 exponent = v & 0x7c00u;
    const bool isDenormal = exponent == 0;
    exponent = ((exponent >> 3) + 14336u) & 0xffffu;
    const u32 corrHigh = isDenormal ? (signBits | 14336u) : 0u;
    const u32 highBits = signBits | exponent | (mantissa >> 3);
    const u32 lowBits = (mantissa << 13) & 0xffffu;
    return __uint_as_float((highBits << 16) | lowBits) - __uint_as_float(corrHigh << 16);
}

// For every finite non-negative half pattern (all the unsigned format ever sees: inputs are
// clamped to [0, 0x7BFF], reconstructions to <= 31743) the function above equals the hardware
// conversion, except that it halves denormals (exponent field 0) -- checked exhaustively.  Outside the claim: pattern 0x8000
// (the conversion keeps -0, the bit manipulation gives +0) and exponent field 31 (infinities and NaNs against 65536 ... 131008).
template <bool SIGNED>
__device__ __forceinline__ float twosCLHalfToFloat(int v16)
{
    if (SIGNED)
        return twosCLHalfToFloatBits(v16);
    const float f = __half2float(__ushort_as_half((unsigned short)v16));
    return (v16 & 0x7c00) ? f : f * 0.5f;
}

// ReconstructHDR{Signed,Unsigned}Uninverted for one channel, IndexSelectorHDR.h:34-66
// (64 - w) * e0 + w * e1 = 64 * e0 + w * (e1 - e0): one 24-bit multiply-add per interpolant instead of two 32-bit
// multiplications (quarter rate on gfx950) -- |e| < 2^16, w <= 64, so every term fits 24 bits
// reconstructBase: 64 * e0 + 32, with the difference e1 - e0 computed once per round and channel
__device__ __forceinline__ u32 mulU24(u32 a, u32 b)
{
    u32 r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// DYN: the weight is a run-time value (forced v_mad_i32_i24); otherwise a literal the compiler may fold
template <bool SIGNED, bool DYN = true>
__device__ __forceinline__ int reconstructFrom(int base, int diff, int weight)
{
    if (SIGNED)
    {
        int p = (DYN ? madI24(weight, diff, base) : mad24(weight, diff, base)) >> 6;
        p = p > 32767 ? 32767 : (p < -32768 ? -32768 : p);
        const bool neg = p < 0;
        const int a = neg ? -p : p;
        int scaled = (int)(__umul24((u32)a & 0xffffu, 31u) >> 5); // UnscaleHDRValueSigned, BC67.cpp:766-782
        scaled = scaled > 32767 ? 32767 : scaled;
        return (int)(short)(unsigned short)((u32)scaled | (neg ? 0x8000u : 0u));
    }
    else
    {
        // e < 2^16, weight <= 64: 0 <= 64 e0 + w (e1 - e0) + 32 < 2^22 + 32, so ">> 6 & 0xffff" is one v_bfe_u32 (and the mask never bites)
        const u32 p = __builtin_amdgcn_ubfe((u32)(DYN ? madI24(weight, diff, base) : mad24(weight, diff, base)), 6u, 16u);
        return (int)(mulU24(p, 31u) >> 6);   // UnscaleHDRValueUnsigned
    }
}
template <bool SIGNED>
__device__ __forceinline__ int reconstructChannel(int e0, int e1, int weight)
{
    return reconstructFrom<SIGNED, false>(e0 * 64 + 32, e1 - e0, weight);
}

// A mode of a precision as one word (modeWord in the kernel): mode | transformed << 4 | the bits a delta loses per channel
// (16 - its stored width) << 8, 16, 24
__device__ __forceinline__ int lostBitsOf(u32 mw, int ch) { return (int)((mw >> (8 + 8 * ch)) & 31u); }
// the delta v - base as a transformed mode stores it: 16-bit arithmetic, sign-extended from the 16 - lost bits it keeps
__device__ __forceinline__ int deltaOf(int v, int base, int lost)
{
    const int d16 = (int)(short)(unsigned short)(v - base);
    return (int)(short)(unsigned short)((u32)d16 << lost) >> lost;
}
// Evaluate*Legality for one value, BC67.cpp:2597-2663: does base + the stored delta give v back in the mask = 2^aPrec - 1 bits?
__device__ __forceinline__ bool deltaFits(u32 mw, int v, int base, int ch, int mask)
{
    return ((deltaOf(v, base, lostBitsOf(mw, ch)) + base) & mask & 0xffff) == (v & mask & 0xffff);
}

// the 32-lane slice of a wave ballot that belongs to the lane's reference group (8 blocks x 4 sub-lanes)
__device__ __forceinline__ u32 groupBits(u64 ballot, int lane) { return (u32)(ballot >> (lane & 32)); }
// v_mov_b32 with a DPP quad_perm: the lanes of every quad rearranged (no LDS traffic, no address register)
template <int PERM>
__device__ __forceinline__ u32 quadPerm(u32 v)
{
    return (u32)__builtin_amdgcn_mov_dpp((int)v, PERM, 0xf, 0xf, true);
}
// the value sub-lane Q of the lane's quad holds
template <int Q>
__device__ __forceinline__ u32 quadBcast(u32 v) { return quadPerm<Q * 0x55>(v); }
// OR / minimum over the lane's quad, in all four lanes: neighbours exchanged (quad_perm [1,0,3,2]), then the pairs ([2,3,0,1])
__device__ __forceinline__ u32 quadOr(u32 v)
{
    v |= quadPerm<0xb1>(v);
    v |= quadPerm<0x4e>(v);
    return v;
}
__device__ __forceinline__ float quadMin(float v)
{
    float o = __uint_as_float(quadPerm<0xb1>(__float_as_uint(v)));
    v = o < v ? o : v;
    o = __uint_as_float(quadPerm<0x4e>(__float_as_uint(v)));
    v = o < v ? o : v;
    return v;
}
// meta round m = 3 * tweak + refine pass: its tweak (m = 0 ... 11)
__device__ __forceinline__ int tweakOf(int m) { return (m * 11) >> 5; }
} // namespace
