// BC7 dual-plane modes 4 / 5: one (mode, rotation, index selector) configuration per lane quad (evalDual).
// Part of bc7_kernel.hip (one translation unit), included after bc7_chain.h.
#pragma once
#include "bc7_dual_setup.h"

namespace
{
// In-place channel rotation of the packed pixels: rotation r > 0 exchanges channel r-1 with
// alpha (reference BC67.cpp:1695-1698).  The exchange is an involution.
__device__ __forceinline__ u32 rotatePixel(u32 pk, int rotation)
{
    if (rotation == 1) return (pk & 0x00ffff00u) | (pk >> 24) | (pk << 24);
    if (rotation == 2) return (pk & 0x00ff00ffu) | ((pk >> 16) & 0x0000ff00u) | ((pk << 16) & 0xff000000u);
    if (rotation == 3) return (pk & 0x0000ffffu) | ((pk >> 8) & 0x00ff0000u) | ((pk << 8) & 0xff000000u);
    return pk;
}

struct DualInv
{
    const u32 *words; // s_raw + block index
    int rowSq[4], rowVs[4];
    u32 minMax;
};

// One group of four pixels (16 bytes) of the block's copy in LDS, at the byte address `addr` of the LDS segment.
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ldsQuad(u32 addr)
{
    const u32x4 v = *(const __attribute__((address_space(3))) u32x4 *)(size_t)addr;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// One (mode, rotation, index selector) configuration of the dual-plane modes 4/5 (reference BC67.cpp:1725-1940): sub-lane
// c runs seed point c.  rw / rwSq / rrcpW are rotated so that position 3 is the separately coded channel.  The seeds, the
// float index selection and the refiner are the reference's, operation for operation, and the same for fast and slow
// indexing (Flags::Better / Ultra: the two neighbours of every index are probed as well); the pixel loop and the error
// sum are each path's own.
// Invariants of the block in rotated channel order (DualInv): sum(px^2) per channel, min / max of the separately coded
// channel, and the refiner's sums of the pre-weighted pixels sum(x * w) -- ContributeUnweightedPW adds the same 16 values
// in the same order whatever the indexes are (EndpointRefiner.h:78-92), so the sum is taken once per block.
// They wait in LDS (rows of 16 words, one word per block of the wave) and are read where they are used -- the pixel loop of
// the search is the place with the fewest registers to spare: `rowSq[ch]` / `rowVs[ch]` = word offset of channel position
// ch's sum(px^2) / refiner sum, `minMax` = min | max << 8 of the separately coded channel.
// `sP`: the block's pixels in LDS, already in rotated channel order, read again in every round (one 128-bit load per
// group g of four pixels) instead of living in 16 registers.
// FAST: channel-major, four words (channel positions 0..3, one byte per pixel) per group.  The integer error
// sum(rec - px)^2 is evaluated per channel as sum(rec^2) - 2 sum(rec * px) + sum(px^2) with the reconstructed bytes looked
// up by v_perm_b32 from the level table and the sums taken by v_dot4_u32_u8 over four pixels at a time -- integers, so
// the result is the same number.
// !FAST: one packed word per pixel (byte 3 = the separately coded channel).
template <bool FAST>
__device__ __forceinline__ void evalDual(const u32 *sP, const DualInv &inv, int mode, int indexSelector, const Unfinished &uRGB,
                                         int numTweak, const float (&rw)[4], const float (&rwSq)[4],
                                         const float (&rrcpW)[4], u32 flags, const CvttDeviceTables *__restrict__ T,
                                         int numRefine, int lane, ShapeBest &bestRGB, ShapeBest &bestA)
{
    const int c = lane & 3;
    int rgbPrec, alphaPrec;
    if (mode == 4)
    {
        rgbPrec = indexSelector ? 3 : 2;
        alphaPrec = indexSelector ? 2 : 3;
    }
    else
        rgbPrec = alphaPrec = 2;
    const int rgbRange = 1 << rgbPrec, alphaRange = 1 << alphaPrec;
    const float rgbMax = (float)(rgbRange - 1), alphaMaxV = (float)(alphaRange - 1);
    const float rgbRcpMax = T->rcpMaxIndex[rgbPrec], alphaRcpMax = T->rcpMaxIndex[alphaPrec];
    const float wRcp16 = T->rcpTable[16];
    const bool uniformErr = (flags & CVTTMI_FLAG_UNIFORM) != 0;

    bestRGB.err = bestA.err = FLT_MAX;
    bestRGB.ep0 = bestRGB.ep1 = bestRGB.idxLo = bestRGB.idxHi = 0;
    bestA.ep0 = bestA.ep1 = bestA.idxLo = bestA.idxHi = 0;

    const int alphaMin = (int)(inv.minMax & 0xffu), alphaMax = (int)(inv.minMax >> 8);

    const int tweak = c;
    if (tweak < numTweak)
    {
        int ep[2][4];
        {
            const float tf0 = T->tweakFactors[rgbPrec - 2][tweak][0];
            const float tf1 = T->tweakFactors[rgbPrec - 2][tweak][1];
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
            {
                ep[0][ch] = endpointByte(uRGB.base[ch] + uRGB.offset[ch] * tf0);
                ep[1][ch] = endpointByte(uRGB.base[ch] + uRGB.offset[ch] * tf1);
            }
            // TweakAlpha (reference BC67.cpp:815-827)
            const float af0 = T->tweakFactors[alphaPrec - 2][tweak][0];
            const float af1 = T->tweakFactors[alphaPrec - 2][tweak][1];
            const float base = (float)alphaMin;
            const float offs = (float)alphaMax - base;
            ep[0][3] = endpointByte(base + offs * af0);
            ep[1][3] = endpointByte(base + offs * af1);
        }

        for (int refine = 0; refine < numRefine; refine++)
        {
            const bool last = (refine == numRefine - 1);
            // CompressEndpoints4 / 5 (reference BC67.cpp:901-923)
            const int cb = (mode == 4) ? 5 : 7;
#pragma unroll
            for (int j = 0; j < 2; j++)
            {
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                    ep[j][ch] = unquantize(quantizeNoP(ep[j][ch], cb), cb);
                if (mode == 4)
                    ep[j][3] = unquantize(quantizeNoP(ep[j][3], 6), 6);
            }

            // IndexSelector<3> (rotated weights) and IndexSelector<1> (weight 1.0)
            float origin[4], axis[4];
            // the 4 / 8 values an index can reconstruct, per channel, as bytes
            u32 tabLo[4], tabHi[4];
            {
                float epDW[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                {
                    origin[ch] = (float)ep[0][ch];
                    epDW[ch] = ((float)ep[1][ch] - origin[ch]) * rw[ch];
                }
                float lenSq = epDW[0] * epDW[0];
                lenSq = lenSq + epDW[1] * epDW[1];
                lenSq = lenSq + epDW[2] * epDW[2];
                lenSq = safeDenom(lenSq);
                const float mvdls = rgbMax / lenSq;
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                    axis[ch] = epDW[ch] * rw[ch] * mvdls;
                origin[3] = (float)ep[0][3];
                const float aDW = (float)ep[1][3] - origin[3];
                const float aLen = safeDenom(aDW * aDW);
                axis[3] = aDW * (alphaMaxV / aLen);
                dualLevelTables(ep, rgbPrec == 3, alphaPrec == 3, tabLo, tabHi);
            }
            const v2f org01 = {origin[0], origin[1]}, org23 = {origin[2], origin[3]};
            const v2f ax01 = {axis[0], axis[1]}, ax23 = {axis[2], axis[3]};
            const v2f w01 = {rw[0], rw[1]}, w23 = {rw[2], 1.0f};
            const v2f rcpMax2 = {rgbRcpMax, alphaRcpMax};

            // the error accumulators of either path.  (Declared here, ahead of the refiner's sums, for both: the order of the
            // declarations is the order of the values the slow path's rolled pixel loop carries, and its register assignment
            // follows it.)
            u32 s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0}; // fast indexing: sum(rec * px), sum(rec^2) per channel
            float slowRGB = 0.0f, slowA = 0.0f;               // slow indexing: the error of the chosen candidates
            // the refiner's sums.  Fast indexing starts them from pixel 0's contribution (below) and leaves them unset in the last
            // round, which neither writes nor reads them
            v2f tv01, tv23;
            v2f tt2, ts2; // {RGB plane, alpha plane}
            if constexpr (!FAST)
            {
                tv01 = tv23 = v2f{0.0f, 0.0f};
                tt2 = ts2 = v2f{0.0f, 0.0f};
            }
            u32 rgbLo = 0, rgbHi = 0, aLo = 0, aHi = 0; // 4 bits per pixel, pixel p in slot dualIndexSlot(p)

            // an address the optimiser cannot see through: the loads stay inside the round (hoisted, they would hold 16
            // registers again, and the 64 conversions with them).  What is hidden is the 32-bit LDS address, not a generic
            // pointer, so the loads stay ds_read_b128: no 64-bit address pair, no vmcnt wait, no trip down the vector-memory path
            u32 sPr = (u32)(size_t)(const __attribute__((address_space(3))) u32 *)sP;
            asm volatile("" : "+v"(sPr));
            float errorRGB, errorA;
            if constexpr (FAST)
            {
                u32 iRprev = 0, iAprev = 0; // the even group's index bytes, until the odd group's join them
#pragma unroll
                for (int g = 0; g < 4; g++)
                {
                    u32 iR4 = 0, iA4 = 0;
                    const uint4 L = ldsQuad(sPr + 16u * (u32)g);
                    const u32 Pg[4] = {L.x, L.y, L.z, L.w};
#pragma unroll
                    for (int k = 0; k < 4; k++)
                    {
                        const v2f x01 = {byteF(Pg[0], k), byteF(Pg[1], k)}, x23 = {byteF(Pg[2], k), byteF(Pg[3], k)};
                        const v2f p01 = (x01 - org01) * ax01, p23 = (x23 - org23) * ax23;
                        float dist = p01.x + p01.y;
                        dist = dist + p23.x;
                        // clampRound in two halves.  The last round's index goes to v_cvt_pk_u8_f32 alone, which rounds to nearest even
                        // and saturates at 0 itself: the upper clamp is all it needs (clampHigh, cvtt_kernel_common.h).  The other
                        // rounds' index also weights the refiner and takes the rest: clampRound(v, hi) = rintf(fmaxf(clampHigh(v, hi), 0)),
                        // the rounding first (roundClampLow: the same bits, one v_max_f32 less per index).
                        float fRGB = clampHigh(dist, rgbMax);
                        float fA = clampHigh(p23.y, alphaMaxV);
                        if (!last)
                        {
                            fRGB = roundClampLow(fRGB);
                            fA = roundClampLow(fA);
                        }
                        // the indexes are small integers: v_cvt_pk_u8_f32 converts and files one as byte k in one instruction
                        iR4 = __builtin_amdgcn_cvt_pk_u8_f32(fRGB, (u32)k, iR4);
                        iA4 = __builtin_amdgcn_cvt_pk_u8_f32(fA, (u32)k, iA4);
                        if (!last)
                        {
                            // EndpointRefiner<3> with the rotated weights and EndpointRefiner<1> with weight 1; the sums of the
                            // pre-weighted pixels themselves (vs) do not depend on the indexes: DualInv
                            const v2f f2 = {fRGB, fA};
                            const v2f t2 = f2 * rcpMax2;
                            const v2f tt = {t2.x, t2.x};
                            const v2f v01 = x01 * w01, v23 = x23 * w23;
                            if (g == 0 && k == 0)
                            {
                                // Pixel 0 starts the sums instead of being added to +0: no v_add_f32 0, x (which IEEE forbids the
                                // compiler to drop) and no zeroing.  t2 >= +0 (roundClampLow gives +0 or more, rcpMax2 > 0), so
                                // t2 * t2 and t2 are >= +0 and 0 + x is x bit for bit; so is tt * v with weights >= +0, and a NaN
                                // product is quiet already.  Only a negative (or -0) weight can make tt * v a -0 that 0 + x would turn
                                // into +0.  The sum then still differs only while every later term is -0 as well (one +0 or non-zero
                                // term and both forms agree), so as -0 for +0, and that sign ends in the solve: with
                                // z = ts * vs * wRcp16, tv - z is -z for z != 0 and +0 for z = -0 either way; for z = +0 (vs = +0) the
                                // quotient a = +-0 leaves b = (vs - a * ts) * wRcp16 = +0 and a + b = +0, the two end points.
                                tv01 = tt * v01;
                                tv23 = t2 * v23;
                                tt2 = t2 * t2;
                                ts2 = t2;
                            }
                            else
                            {
                                tv01 = tv01 + tt * v01;
                                tv23 = tv23 + t2 * v23;
                                tt2 = tt2 + t2 * t2;
                                ts2 = ts2 + t2;
                            }
                        }
                    }
                    // the bytes as they are, the odd group in the high nibbles (dualIndexSlot): every index is below 8
                    if (g & 1)
                    {
                        (g == 1 ? rgbLo : rgbHi) = iRprev | (iR4 << 4);
                        (g == 1 ? aLo : aHi) = iAprev | (iA4 << 4);
                    }
                    else
                    {
                        iRprev = iR4;
                        iAprev = iA4;
                    }
#pragma unroll
                    for (int ch = 0; ch < 4; ch++)
                    {
                        const u32 R = __builtin_amdgcn_perm(tabHi[ch], tabLo[ch], ch == 3 ? iA4 : iR4);
                        s1[ch] = __builtin_amdgcn_udot4(R, Pg[ch], s1[ch], false);
                        s2[ch] = __builtin_amdgcn_udot4(R, R, s2[ch], false);
                    }
                }

                u32 err[4];
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                    err[ch] = s2[ch] + inv.words[inv.rowSq[ch]] - 2u * s1[ch];
                if (uniformErr)
                {
                    errorRGB = (float)(int)(err[0] + err[1] + err[2]);
                    errorA = (float)(int)err[3];
                }
                else
                {
                    errorRGB = (float)(int)err[0] * rwSq[0];
                    errorRGB = errorRGB + (float)(int)err[1] * rwSq[1];
                    errorRGB = errorRGB + (float)(int)err[2] * rwSq[2];
                    errorA = (float)(int)err[3] * rwSq[3];
                }
            }
            else
            {
                // four pixels per trip, the trips not unrolled: unrolled sixteen times, the three probes of every pixel kept so
                // much in flight that this instantiation could not be held in the 128 registers of four waves per SIMD
#pragma unroll 1
                for (int g = 0; g < 4; g++)
                {
                    const uint4 L = ldsQuad(sPr + 16u * (u32)g);
                    u32 r4 = 0, a4 = 0; // the group's indexes, one per byte (the fast path's layout: dualIndexSlot)
#pragma unroll
                    for (int k = 0; k < 4; k++)
                    {
                        const u32 pk = k == 0 ? L.x : k == 1 ? L.y : k == 2 ? L.z : L.w;
                        const v2f x01 = {byteF(pk, 0), byteF(pk, 1)}, x23 = {byteF(pk, 2), byteF(pk, 3)};
                        const v2f p01 = (x01 - org01) * ax01, p23 = (x23 - org23) * ax23;
                        float dist = p01.x + p01.y;
                        dist = dist + p23.x;
                        float fRGB = clampRound(dist, rgbMax);
                        float fA = clampRound(p23.y, alphaMaxV);
                        int iRGB = (int)fRGB, iA = (int)fA;

                        // reference BC67.cpp:1834-1880
                        float eRGB = 0.0f, eA = 0.0f;
                        const int c1R = (iRGB > 1 ? iRGB : 1) - 1, c2R = (iRGB + 1 < rgbRange - 1) ? iRGB + 1 : rgbRange - 1;
                        const int c1A = (iA > 1 ? iA : 1) - 1, c2A = (iA + 1 < alphaRange - 1) ? iA + 1 : alphaRange - 1;
                        const u32 selR = (u32)iRGB | ((u32)c1R << 8) | ((u32)c2R << 16) | 0x0c000000u;
                        const u32 selA = (u32)iA | ((u32)c1A << 8) | ((u32)c2A << 16) | 0x0c000000u;
                        // byte k = the value candidate k reconstructs: with the level tables the three candidates of a pixel are
                        // one v_perm_b32 per channel instead of a weight and a multiply-add each
                        const u32 rec0 = __builtin_amdgcn_perm(tabHi[0], tabLo[0], selR), rec1 = __builtin_amdgcn_perm(tabHi[1], tabLo[1], selR),
                                  rec2 = __builtin_amdgcn_perm(tabHi[2], tabLo[2], selR), rec3 = __builtin_amdgcn_perm(tabHi[3], tabLo[3], selA);
                        auto probeOne = [&](auto kTag, int candRGB, int candA) {
                            constexpr int K = decltype(kTag)::value;
                            // (rec - px)^2 as floats: byte -> float conversions, a subtract and a multiply are exact on these
                            // integers (|d| <= 255, d^2 < 2^24), so the squares are the numbers the integer form converts -- and
                            // they are plain f32 instructions, which a second wave can issue alongside (SDWA and 24-bit
                            // multiplies cannot)
                            const float d0 = byteF(rec0, K) - x01.x, d1 = byteF(rec1, K) - x01.y, d2 = byteF(rec2, K) - x23.x, d3 = byteF(rec3, K) - x23.y;
                            const float e3[3] = {d0 * d0, d1 * d1, d2 * d2};
                            const float e1 = d3 * d3;
                            float er, ea;
                            if (uniformErr)
                            {
                                er = (e3[0] + e3[1]) + e3[2];
                                ea = e1;
                            }
                            else
                            {
                                er = e3[0] * rwSq[0];
                                er = er + e3[1] * rwSq[1];
                                er = er + e3[2] * rwSq[2];
                                ea = e1 * rwSq[3];
                            }
                            if (K == 0)
                            {
                                eRGB = er;
                                eA = ea;
                            }
                            else
                            {
                                // (the winner is tracked as an integer and converted once; equal errors are equal bits, so the
                                // comparison that moves the index also serves the minimum)
                                const bool bR = er < eRGB, bA = ea < eA;
                                eRGB = bR ? er : eRGB;
                                eA = bA ? ea : eA;
                                iRGB = bR ? candRGB : iRGB;
                                iA = bA ? candA : iA;
                            }
                        };
                        probeOne(std::integral_constant<int, 0>{}, iRGB, iA);
                        probeOne(std::integral_constant<int, 1>{}, c1R, c1A);
                        probeOne(std::integral_constant<int, 2>{}, c2R, c2A);
                        fRGB = (float)iRGB;
                        fA = (float)iA;
                        slowRGB = slowRGB + eRGB;
                        slowA = slowA + eA;

                        if (!last)
                        {
                            // EndpointRefiner<3> with the rotated weights and EndpointRefiner<1> with weight 1
                            const v2f f2 = {fRGB, fA};
                            const v2f t2 = f2 * rcpMax2;
                            const v2f tt = {t2.x, t2.x};
                            const v2f v01 = x01 * w01, v23 = x23 * w23;
                            tv01 = tv01 + tt * v01;
                            tv23 = tv23 + t2 * v23;
                            tt2 = tt2 + t2 * t2;
                            ts2 = ts2 + t2;
                        }
                        r4 |= (u32)iRGB << (8 * k);
                        a4 |= (u32)iA << (8 * k);
                    }
                    if (g < 2)
                    {
                        rgbLo |= r4 << (4 * g);
                        aLo |= a4 << (4 * g);
                    }
                    else
                    {
                        rgbHi |= r4 << (4 * (g - 2));
                        aHi |= a4 << (4 * (g - 2));
                    }
                }
                errorRGB = slowRGB;
                errorA = slowA;
            }

            if (errorRGB < bestRGB.err)
            {
                bestRGB.err = errorRGB;
                bestRGB.ep0 = (u32)ep[0][0] | ((u32)ep[0][1] << 8) | ((u32)ep[0][2] << 16);
                bestRGB.ep1 = (u32)ep[1][0] | ((u32)ep[1][1] << 8) | ((u32)ep[1][2] << 16);
                bestRGB.idxLo = rgbLo;
                bestRGB.idxHi = rgbHi;
            }
            if (errorA < bestA.err)
            {
                bestA.err = errorA;
                bestA.ep0 = (u32)ep[0][3] << 24;
                bestA.ep1 = (u32)ep[1][3] << 24;
                bestA.idxLo = aLo;
                bestA.idxHi = aHi;
            }

            if (!last)
            {
                // EndpointRefiner<3> / <1>::GetRefinedEndpointsLDR, 16 contributions each
                const float tv[4] = {tv01.x, tv01.y, tv23.x, tv23.y};
                const float vs[4] = {__builtin_bit_cast(float, inv.words[inv.rowVs[0]]), __builtin_bit_cast(float, inv.words[inv.rowVs[1]]),
                                     __builtin_bit_cast(float, inv.words[inv.rowVs[2]]), __builtin_bit_cast(float, inv.words[inv.rowVs[3]])};
                {
                    const float ttRGB = tt2.x, tsRGB = ts2.x;
                    float adenom = (ttRGB * 16.0f - tsRGB * tsRGB) * wRcp16;
                    const bool z = (adenom == 0.0f);
                    if (z) adenom = 1.0f;
#pragma unroll
                    for (int ch = 0; ch < 3; ch++)
                    {
                        const float a = (tv[ch] - tsRGB * vs[ch] * wRcp16) / adenom;
                        const float b = (vs[ch] - a * tsRGB) * wRcp16;
                        float p1 = b, p2 = a + b;
                        if (z)
                        {
                            p1 = vs[ch] * wRcp16;
                            p2 = p1;
                        }
                        ep[0][ch] = endpointByte(p1 * rrcpW[ch]);
                        ep[1][ch] = endpointByte(p2 * rrcpW[ch]);
                    }
                }
                {
                    const float ttA = tt2.y, tsA = ts2.y;
                    float adenom = (ttA * 16.0f - tsA * tsA) * wRcp16;
                    const bool z = (adenom == 0.0f);
                    if (z) adenom = 1.0f;
                    const float a = (tv[3] - tsA * vs[3] * wRcp16) / adenom;
                    const float b = (vs[3] - a * tsA) * wRcp16;
                    float p1 = b, p2 = a + b;
                    if (z)
                    {
                        p1 = vs[3] * wRcp16;
                        p2 = p1;
                    }
                    ep[0][3] = endpointByte(p1);
                    ep[1][3] = endpointByte(p2);
                }
            }
        }
    }
    quadArgminBroadcast(bestRGB, lane);
    quadArgminBroadcast(bestA, lane);
}

} // namespace
