// ETC error metrics and block emitters: the fake-BT.709 conversion and its rounding resolvers, EtcErr (uniform / weighted /
// fake-BT.709, one colour or two at a time), planarDecode and the T / H mode emitters.  Part of etc2_kernel.hip (one
// translation unit), included after etc2_wave.h.
#pragma once

namespace
{
// ConvertToFakeBT709, ETC.cpp:2343-2352
__device__ __forceinline__ void toFake709(float (&yuv)[3], float r, float g, float b)
{
    yuv[0] = r * 0.368233989135369f + g * 1.23876274963149f + b * 0.125054068802017f;
    yuv[1] = r * 0.5f - g * 0.4541529f - b * 0.04584709f;
    yuv[2] = r * -0.081014709086133f - g * 0.272538676238785f + b * 0.353553390593274f;
}

// the octant search shared by ResolveTHFakeBT709Rounding and ResolveHalfBlockFakeBT709RoundingAccurate
// (ETC.cpp:2199-2231, 2304-2326): which of the 8 cell corners is nearest to `target`; the reference's error adds the
// chroma-U difference twice instead of squaring it
__device__ __forceinline__ int fakeOctant(const float (&lowF)[3], const float (&highF)[3], const float (&target)[3])
{
    float cum[3];
    toFake709(cum, target[0], target[1], target[2]);
    float bestError = FLT_MAX;
    int bestOctant = 0;
#pragma unroll
    for (int octant = 0; octant < 8; octant++)
    {
        float oy[3];
        toFake709(oy, (octant & 1) ? highF[0] : lowF[0], (octant & 2) ? highF[1] : lowF[1], (octant & 4) ? highF[2] : lowF[2]);
        const float d0 = oy[0] - cum[0], d1 = oy[1] - cum[1], d2 = oy[2] - cum[2];
        const float error = d0 * d0 + d1 + d1 + d2 * d2;
        if (error < bestError)
            bestOctant = octant;
        bestError = sseMin(error, bestError);
    }
    return bestOctant;
}

// ResolveTHFakeBT709Rounding, ETC.cpp:2286-2327
__device__ __forceinline__ void resolveTHFake(int (&quantized)[3], const int (&targets)[3], int granularity)
{
    float lowF[3], highF[3], tf[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
    {
        const int unq = (quantized[ch] << 4) | quantized[ch];
        const int next = unq + 17 < 255 ? unq + 17 : 255;
        lowF[ch] = (float)(int)(short)((int)(short)(unq * granularity) << 1);
        highF[ch] = (float)(int)(short)((int)(short)(next * granularity) << 1);
        tf[ch] = (float)targets[ch];
    }
    const int octant = fakeOctant(lowF, highF, tf);
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
        quantized[ch] += (octant >> ch) & 1;
}

// ResolveHalfBlockFakeBT709RoundingAccurate / Fast, ETC.cpp:2157-2284
__device__ __forceinline__ void resolveHalfFake(int (&quantized)[3], const int (&cumulative)[3], bool isDifferential, bool accurate,
                                                const CvttDeviceTables *__restrict__ T)
{
    if (accurate)
    {
        float lowF[3], highF[3], tf[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
        {
            const u32 cu = (u32)cumulative[ch];
            int unq, next;
            if (isDifferential)
            {
                quantized[ch] = (int)(((((cu << 5) - cu) + (cu >> 3)) & 0xffffu) >> 11);
                unq = (quantized[ch] << 3) | (quantized[ch] >> 2);
                const int qn = quantized[ch] + 1 < 31 ? quantized[ch] + 1 : 31;
                next = (qn << 3) | (qn >> 2);
            }
            else
            {
                quantized[ch] = (int)(((((cu << 5) - ((cu << 1) & 0xffffu)) + (cu >> 3)) & 0xffffu) >> 12);
                unq = (quantized[ch] << 4) | quantized[ch];
                next = unq + 17 < 255 ? unq + 17 : 255;
            }
            lowF[ch] = (float)(unq << 3);
            highF[ch] = (float)(next << 3);
            tf[ch] = (float)cumulative[ch];
        }
        const int octant = fakeOctant(lowF, highF, tf);
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            quantized[ch] += (octant >> ch) & 1;
        return;
    }
    int fill[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
        fill[ch] = cumulative[ch] + (cumulative[ch] >> 8);
    const int index = isDifferential ? (((fill[0] << 6) & 0xf00) | ((fill[1] << 4) & 0x0f0) | ((fill[2] >> 2) & 0x00f))
                                     : (((fill[0] << 5) & 0xf00) | ((fill[1] << 1) & 0x0f0) | ((fill[2] >> 3) & 0x00f));
    const int octant = T->fake709Rounding[index];
    const int upper = isDifferential ? 31 : 15, shift = isDifferential ? 6 : 7;
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
    {
        const int q = (fill[ch] >> shift) + ((octant >> ch) & 1);
        quantized[ch] = q < upper ? q : upper;
    }
}

struct EtcErr
{
    bool uniform;
    float rw, gw, bw;
    bool fake;
    // the metric of most call sites: ComputeErrorFakeBT709 (ETC.cpp:82-92) first, then uniform, then weighted
    __device__ __forceinline__ float operator()(int r, int g, int b, const int *px, const float *pw) const
    {
        if (fake)
        {
            float yuv[3];
            toFake709(yuv, (float)r, (float)g, (float)b);
            const float dy = yuv[0] - pw[0], du = yuv[1] - pw[1], dv = yuv[2] - pw[2];
            return dy * dy + du * du + dv * dv;
        }
        return wu(r, g, b, px, pw);
    }
    // The weighted metric for TWO colours at once (a v2f, cvtt_kernel_common.h: two plain f32 instructions per operation): each
    // of the two does ComputeErrorWeighted's operations in its order (product, difference, squares added left to right), so both
    // results are the numbers the scalar form gives.  Only valid when !uniform (and, where the caller would use operator(), !fake).
    __device__ __forceinline__ void weigh2(v2f (&mw)[3], const int (&a)[3], const int (&b)[3]) const
    {
        mw[0] = v2f{(float)a[0] * rw, (float)b[0] * rw};
        mw[1] = v2f{(float)a[1] * gw, (float)b[1] * gw};
        mw[2] = v2f{(float)a[2] * bw, (float)b[2] * bw};
    }
    __device__ __forceinline__ v2f err2(const v2f (&mw)[3], const float *pw) const
    {
        v2f d = mw[0] - v2f{pw[0], pw[0]};
        v2f e = d * d;
        d = mw[1] - v2f{pw[1], pw[1]};
        e = e + d * d;
        d = mw[2] - v2f{pw[2], pw[2]};
        e = e + d * d;
        return e;
    }
    // ComputeErrorUniform / ComputeErrorWeighted, ETC.cpp:59-80.  The line colours of the T modes are measured with
    // this even under ETC_UseFakeBT709 (ETC.cpp:600, 1133, 1150), against pre-weighted pixels that then hold luma/chroma
    __device__ __forceinline__ float wu(int r, int g, int b, const int *px, const float *pw) const
    {
        if (uniform)
        {
            const float d0 = (float)(r - px[0]), d1 = (float)(g - px[1]), d2 = (float)(b - px[2]);
            float e = d0 * d0;
            e = e + d1 * d1;
            e = e + d2 * d2;
            return e;
        }
        const float dr = (float)r * rw - pw[0];
        const float dg = (float)g * gw - pw[1];
        const float db = (float)b * bw - pw[2];
        return dr * dr + dg * dg + db * db;
    }
};

__device__ __forceinline__ int planarDecode(int coeff, int ch)
{
    return (ch == 1) ? (((coeff << 1) | (coeff >> 6)) & 0xffff) : (((coeff << 2) | (coeff >> 4)) & 0xffff);
}

// EmitTModeBlock, ETC.cpp:2414-2460
__device__ __forceinline__ void emitT(u32 &hi, u32 &lo, const int (&lineColor)[3], const int (&iso)[3], u32 packedSelectors, int table, bool opaque = true)
{
    hi = 0;
    lo = 0;
    const int rh = (iso[0] >> 2) & 3, rl = iso[0] & 3;
    if (rh + rl < 4) hi |= 1u << (58 - 32); else hi |= 7u << (61 - 32);
    hi |= (u32)rh << (59 - 32);
    hi |= (u32)rl << (56 - 32);
    hi |= (u32)iso[1] << (52 - 32);
    hi |= (u32)iso[2] << (48 - 32);
    hi |= (u32)lineColor[0] << (44 - 32);
    hi |= (u32)lineColor[1] << (40 - 32);
    hi |= (u32)lineColor[2] << (36 - 32);
    hi |= (u32)((table >> 1) & 3) << (34 - 32);
    if (opaque)
        hi |= 1u << (33 - 32);
    hi |= (u32)(table & 1);
#pragma unroll
    for (int px = 0; px < 16; px++)
    {
        const int src = ((px & 3) << 2) | (px >> 2); // selectorOrder
        const u32 sel = (packedSelectors >> (2 * src)) & 3u;
        lo |= (sel & 1u) << px;
        lo |= ((sel >> 1) & 1u) << (16 + px);
    }
}

// EmitHModeBlock, ETC.cpp:2462-2563.  bc0 / bc1: 4:4:4 colours packed r << 10 | g << 5 | b.
__device__ __forceinline__ void emitH(u32 &outHi, u32 &outLo, int bc0, int bc1, u32 sectorBits, u32 signBits, int table, bool opaque)
{
    if (bc0 == bc1)
    {
        const int lineColor[3] = {(bc0 >> 10) & 0x1f, (bc0 >> 5) & 0x1f, bc0 & 0x1f};
        u32 packedSelectors = 0x55555555u;
#pragma unroll
        for (int px = 0; px < 16; px++)
            packedSelectors |= ((signBits >> px) & 1u) << ((px * 2) + 1);
        emitT(outHi, outLo, lineColor, lineColor, packedSelectors, table, opaque);
        return;
    }
    int colors[2][3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
    {
        colors[0][ch] = (bc0 >> ((2 - ch) * 5)) & 15;
        colors[1][ch] = (bc1 >> ((2 - ch) * 5)) & 15;
    }
    if (((table & 1) == 1) != (bc0 > bc1))
    {
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
        {
            const int t = colors[0][ch];
            colors[0][ch] = colors[1][ch];
            colors[1][ch] = t;
        }
        sectorBits ^= 0xffffu;
    }
    const int r1 = colors[0][0], g1a = colors[0][1] >> 1, g1b = colors[0][1] & 1, b1a = colors[0][2] >> 3, b1b = colors[0][2] & 7;
    const int r2 = colors[1][0], g2 = colors[1][1], b2 = colors[1][2];
    u32 hi = 0, lo = 0;
    if ((g1a & 4) != 0 && r1 + g1a < 8) hi |= 1u << (63 - 32);
    const int fakeDG = b1b >> 1, fakeG = b1a | (g1b << 1);
    if (fakeG + fakeDG < 4) hi |= 1u << (50 - 32); else hi |= 7u << (53 - 32);
    hi |= (u32)r1 << (59 - 32);
    hi |= (u32)g1a << (56 - 32);
    hi |= (u32)g1b << (52 - 32);
    hi |= (u32)b1a << (51 - 32);
    hi |= (u32)b1b << (47 - 32);
    hi |= (u32)r2 << (43 - 32);
    hi |= (u32)g2 << (39 - 32);
    hi |= (u32)b2 << (35 - 32);
    hi |= (u32)((table >> 2) & 1) << (34 - 32);
    if (opaque)
        hi |= 1u << (33 - 32);
    hi |= (u32)((table >> 1) & 1);
#pragma unroll
    for (int px = 0; px < 16; px++)
    {
        const int src2 = ((px & 3) << 2) | (px >> 2);
        lo |= ((signBits >> src2) & 1u) << px;
        lo |= ((sectorBits >> src2) & 1u) << (16 + px);
    }
    outHi = hi;
    outLo = lo;
}
} // namespace
