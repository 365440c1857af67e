// The texel decoders of every format (include/cvtt_mi355x.h, CVTTMI_FMT_*), one lane per block and integer-only: a packed
// block's 8 or 16 bytes -> its 16 texels in registers (decodeTexels<F>).  decode_kernel.hip stores them or measures them
// against a source; nothing here knows about lanes or memory beyond the block's own load.  BC7 and BC6H follow
// cvtt::Kernels::DecodeBC7 / DecodeBC6HU / DecodeBC6HS (reference ConvectionKernels_API.cpp:288-310 ->
// BC7Computer::UnpackOne, ConvectionKernels_BC67.cpp:2206-2423, and BC6HComputer::UnpackOne, 3058-3289): a block with a
// reserved mode decodes to zeros (BC7) / zeros with alpha 1.0 (BC6H), like the reference.  The other formats: INTEGRATION.md,
// "Decoding and measuring every format", with the reference lines each rule follows; numpy restatement:
// tests/texture_decode_ref.py.
#ifndef CVTTMI_DECODE_TEXELS_H
#define CVTTMI_DECODE_TEXELS_H
#include "cvtt_kernel_common.h"
#include "texture_formats.h"

namespace
{
// what the kernels ask of a format: its row of kCvttTextureFormats at compile time
template <int F> struct Fmt
{
    static constexpr CvttTextureFormat row = kCvttTextureFormats[F];
    static constexpr bool hdr = row.cls == kCvttHalfRgb;
    static constexpr bool r11 = row.cls == kCvttR11;
    static constexpr bool snorm = row.cls == kCvttSnorm8;
    static constexpr bool image = row.image != kCvttNoImage;
    static constexpr u32 bcBytes = row.bcBytes;
    static constexpr u32 texBytes = row.texBytes;
    static constexpr u32 mask = row.mask;
};

struct BitReader
{
    u64 lo, hi;
    int pos;
    __device__ __forceinline__ u32 get(int bits)
    {
        if (bits <= 0)
            return 0;
        u64 v;
        if (pos < 64)
        {
            v = lo >> pos;
            if (pos + bits > 64)
                v |= hi << (64 - pos);
        }
        else
            v = hi >> (pos - 64);
        pos += bits;
        return (u32)(v & ((1ull << bits) - 1ull));
    }
};

__device__ __forceinline__ int bc7Weight(int indexBits, int index)
{
    // g_weightTables as g_weightReciprocals (IndexSelector.cpp:43-62): identical values
    const int range = 1 << indexBits;
    const int rcp = (65536 + (range - 1)) / (2 * (range - 1));
    return (rcp * index + 256) >> 9;
}

// one BC7 block -> 16 RGBA8 texels (R in the low byte)
__device__ __forceinline__ void bc7Block(const uint4 raw, const CvttDeviceTables *__restrict__ T, u32 pixels[16])
{
    BitReader br = {((u64)raw.y << 32) | raw.x, ((u64)raw.w << 32) | raw.z, 0};

    int mode = 8;
    for (int i = 0; i < 8; i++)
        if (br.get(1) == 1)
        {
            mode = i;
            break;
        }
    if (mode > 7)
    {
        for (int px = 0; px < 16; px++)
            pixels[px] = 0;
        return;
    }
    // mode table of the format (reference BC67.cpp:108-123)
    const int numSubsetsTab[8] = {3, 2, 3, 2, 1, 1, 1, 2};
    const int partitionBitsTab[8] = {4, 6, 6, 6, 0, 0, 0, 6};
    const int rgbBitsTab[8] = {4, 6, 5, 7, 5, 7, 7, 5};
    const int alphaBitsTab[8] = {0, 0, 0, 0, 6, 8, 7, 5};
    const int indexBitsTab[8] = {3, 3, 2, 2, 2, 2, 4, 2};
    const int alphaIndexBitsTab[8] = {0, 0, 0, 0, 3, 2, 0, 0};
    const int pBitModeTab[8] = {0, 1, 2, 0, 2, 2, 0, 0}; // 0 per endpoint, 1 per subset, 2 none
    int numSubsets = 1, partitionBits = 0, rgbBits = 0, alphaBits = 0, indexBits = 0, alphaIndexBits = 0, pBitMode = 2;
#pragma unroll
    for (int m = 0; m < 8; m++)
        if (mode == m)
        {
            numSubsets = numSubsetsTab[m];
            partitionBits = partitionBitsTab[m];
            rgbBits = rgbBitsTab[m];
            alphaBits = alphaBitsTab[m];
            indexBits = indexBitsTab[m];
            alphaIndexBits = alphaIndexBitsTab[m];
            pBitMode = pBitModeTab[m];
        }
    const bool separateAlpha = (mode == 4 || mode == 5);
    const bool hasAlpha = alphaBits != 0;

    const int partition = (int)br.get(partitionBits);
    const int rotation = separateAlpha ? (int)br.get(2) : 0;
    const int indexSelector = (mode == 4) ? (int)br.get(1) : 0;

    int fix1 = 0, fix2 = 0;
    if (!separateAlpha)
    {
        if (numSubsets == 2)
            fix1 = T->anchor2[partition & 63];
        else if (numSubsets == 3)
        {
            fix1 = T->anchor3[partition & 63][0];
            fix2 = T->anchor3[partition & 63][1];
        }
    }

    int ep[3][2][4];
    for (int ch = 0; ch < 3; ch++)
        for (int s = 0; s < 3; s++)
            for (int e = 0; e < 2; e++)
                ep[s][e][ch] = (s < numSubsets) ? (int)(br.get(rgbBits) << (8 - rgbBits)) : 0;
    for (int s = 0; s < 3; s++)
        for (int e = 0; e < 2; e++)
            ep[s][e][3] = (s < numSubsets && hasAlpha) ? (int)(br.get(alphaBits) << (8 - alphaBits)) : 255;

    int parityBits = 0;
    if (pBitMode != 2)
    {
        for (int s = 0; s < 3; s++)
            if (s < numSubsets)
            {
                int p = 0;
                for (int e = 0; e < 2; e++)
                {
                    if (pBitMode == 0 || e == 0)
                        p = (int)br.get(1);
                    for (int ch = 0; ch < 3; ch++)
                        ep[s][e][ch] |= p << (7 - rgbBits);
                    if (hasAlpha)
                        ep[s][e][3] |= p << (7 - alphaBits);
                }
            }
        parityBits = 1;
    }
    for (int s = 0; s < 3; s++)
        for (int e = 0; e < 2; e++)
        {
            for (int ch = 0; ch < 3; ch++)
                ep[s][e][ch] |= ep[s][e][ch] >> (rgbBits + parityBits);
            if (hasAlpha)
                ep[s][e][3] |= ep[s][e][3] >> (alphaBits + parityBits);
        }

    int idx[16], idx2[16];
    for (int px = 0; px < 16; px++)
    {
        const bool anchor = (px == 0) || (px == fix1) || (px == fix2);
        idx[px] = (int)br.get(indexBits - (anchor ? 1 : 0));
    }
    for (int px = 0; px < 16; px++)
        idx2[px] = separateAlpha ? (int)br.get(alphaIndexBits - (px == 0 ? 1 : 0)) : 0;

    const u32 map2 = T->partition2[partition & 63], map3 = T->partition3[partition & 63];
    for (int px = 0; px < 16; px++)
    {
        int rgbWeight = bc7Weight(indexBits, idx[px]);
        int alphaWeight = 0;
        if (mode == 6 || mode == 7)
            alphaWeight = rgbWeight;
        else if (separateAlpha)
            alphaWeight = bc7Weight(alphaIndexBits, idx2[px]);
        if (indexSelector == 1)
        {
            const int t = rgbWeight;
            rgbWeight = alphaWeight;
            alphaWeight = t;
        }
        int subset = 0;
        if (numSubsets == 2)
            subset = (int)((map2 >> px) & 1u);
        else if (numSubsets == 3)
            subset = (int)((map3 >> (2 * px)) & 3u);
        int e0[4], e1[4];
        for (int ch = 0; ch < 4; ch++)
        {
            e0[ch] = (subset == 0) ? ep[0][0][ch] : (subset == 1) ? ep[1][0][ch] : ep[2][0][ch];
            e1[ch] = (subset == 0) ? ep[0][1][ch] : (subset == 1) ? ep[1][1][ch] : ep[2][1][ch];
        }
        int pixel[4] = {0, 0, 0, 255};
        for (int ch = 0; ch < 3; ch++)
            pixel[ch] = ((64 - rgbWeight) * e0[ch] + rgbWeight * e1[ch] + 32) >> 6;
        if (hasAlpha)
            pixel[3] = ((64 - alphaWeight) * e0[3] + alphaWeight * e1[3] + 32) >> 6;
        if (rotation != 0)
        {
            const int a = pixel[3];
            if (rotation == 1) { pixel[3] = pixel[0]; pixel[0] = a; }
            else if (rotation == 2) { pixel[3] = pixel[1]; pixel[1] = a; }
            else { pixel[3] = pixel[2]; pixel[2] = a; }
        }
        pixels[px] = ((u32)pixel[0] & 0xffu) | (((u32)pixel[1] & 0xffu) << 8) | (((u32)pixel[2] & 0xffu) << 16) | (((u32)pixel[3] & 0xffu) << 24);
    }
}

__device__ __forceinline__ int signExtend(int v, int bits)
{
    if (v & (1 << (bits - 1)))
        v |= -(1 << bits);
    return v;
}

// one BC6H block -> 16 texels of PixelBlockF16 as two words each: (R | G << 16, B | 0x3C00 << 16)
template <bool SIGNED>
__device__ __forceinline__ void bc6hBlock(const uint4 raw, const CvttDeviceTables *__restrict__ T, uint2 dst[16])
{
    BitReader br = {((u64)raw.y << 32) | raw.x, ((u64)raw.w << 32) | raw.z, 0};

    int modeBits = (int)(raw.x & 3u);
    if (modeBits != 0 && modeBits != 1)
        modeBits = (int)(raw.x & 0x1fu);
    int mode = -1;
    for (int m = 0; m < 14; m++)
        if (mode < 0 && T->bc6hModeInfo[m][0] == modeBits)
            mode = m;
    if (mode < 0)
    {
        for (int px = 0; px < 16; px++)
            dst[px] = make_uint2(0u, 0x3c000000u);
        return;
    }
    const bool partitioned = T->bc6hModeInfo[mode][1] != 0;
    const bool transformed = T->bc6hModeInfo[mode][2] != 0;
    const int aPrec = T->bc6hModeInfo[mode][3];
    const int bPrec[3] = {T->bc6hModeInfo[mode][4], T->bc6hModeInfo[mode][5], T->bc6hModeInfo[mode][6]};
    const int headerBits = partitioned ? 82 : 65;

    // header bits -> fields (m d rw rx ry rz gw gx gy gz bw bx by bz), BC6H_IO.cpp via tools/gen_bc6h_layout.py
    u32 fields[14];
    for (int f = 0; f < 14; f++)
        fields[f] = 0;
    for (int bit = 0; bit < headerBits; bit++)
    {
        const u32 b = br.get(1);
        const u32 code = T->bc6hLayout[mode][bit];
        if (code != 255u)
        {
#pragma unroll
            for (int f = 0; f < 14; f++)
                if ((code >> 4) == (u32)f)
                    fields[f] |= b << (code & 15u);
        }
    }
    const int partition = (int)(fields[1] & 31u);
    int eps[2][2][3];
    for (int ch = 0; ch < 3; ch++)
    {
        eps[0][0][ch] = (int)fields[2 + ch * 4 + 0];
        eps[0][1][ch] = (int)fields[2 + ch * 4 + 1];
        eps[1][0][ch] = (int)fields[2 + ch * 4 + 2];
        eps[1][1][ch] = (int)fields[2 + ch * 4 + 3];
    }

    const int fixupIndex1 = partitioned ? (int)T->anchor2[partition] : 0;
    const int indexBits = partitioned ? 3 : 4;
    const int numSubsets = partitioned ? 2 : 1;
    int idx[16];
    for (int px = 0; px < 16; px++)
        idx[px] = (int)br.get((px == 0 || px == fixupIndex1) ? indexBits - 1 : indexBits);

    for (int ch = 0; ch < 3; ch++)
    {
        if (SIGNED)
            eps[0][0][ch] = signExtend(eps[0][0][ch], aPrec);
        if (transformed || SIGNED)
        {
            eps[0][1][ch] = signExtend(eps[0][1][ch], bPrec[ch]);
            if (partitioned)
            {
                eps[1][0][ch] = signExtend(eps[1][0][ch], bPrec[ch]);
                eps[1][1][ch] = signExtend(eps[1][1][ch], bPrec[ch]);
            }
        }
    }
    if (transformed)
    {
        const int wrapMask = (1 << aPrec) - 1;
        for (int ch = 0; ch < 3; ch++)
        {
            eps[0][1][ch] = (eps[0][0][ch] + eps[0][1][ch]) & wrapMask;
            if (SIGNED)
                eps[0][1][ch] = signExtend(eps[0][1][ch], aPrec);
            if (partitioned)
            {
                eps[1][0][ch] = (eps[0][0][ch] + eps[1][0][ch]) & wrapMask;
                eps[1][1][ch] = (eps[0][0][ch] + eps[1][1][ch]) & wrapMask;
                if (SIGNED)
                {
                    eps[1][0][ch] = signExtend(eps[1][0][ch], aPrec);
                    eps[1][1][ch] = signExtend(eps[1][1][ch], aPrec);
                }
            }
        }
    }
    // unquantise
    for (int s = 0; s < 2; s++)
        for (int e = 0; e < 2; e++)
            for (int ch = 0; ch < 3; ch++)
            {
                if (s >= numSubsets)
                    continue;
                int v = eps[s][e][ch];
                if (SIGNED)
                {
                    if (aPrec < 16)
                    {
                        const bool neg = v < 0;
                        const int comp = neg ? -v : v;
                        int unq;
                        if (comp == 0)
                            unq = 0;
                        else if (comp >= ((1 << (aPrec - 1)) - 1))
                            unq = 0x7fff;
                        else
                            unq = ((comp << 15) + 0x4000) >> (aPrec - 1);
                        v = neg ? -unq : unq;
                    }
                }
                else
                {
                    if (aPrec < 15 && v != 0)
                        v = (v == ((1 << aPrec) - 1)) ? 0xffff : (((v << 16) + 0x8000) >> aPrec);
                }
                eps[s][e][ch] = v;
            }

    const u32 map2 = T->partition2[partition];
    for (int px = 0; px < 16; px++)
    {
        const int subset = partitioned ? (int)((map2 >> px) & 1u) : 0;
        const int w = bc7Weight(indexBits, idx[px]);
        u32 c[3];
        for (int ch = 0; ch < 3; ch++)
        {
            const int e0 = subset ? eps[1][0][ch] : eps[0][0][ch], e1 = subset ? eps[1][1][ch] : eps[0][1][ch];
            int comp = ((64 - w) * e0 + w * e1 + 32) >> 6;
            if (SIGNED)
            {
                comp = (comp < 0) ? -(((-comp) * 31) >> 5) : ((comp * 31) >> 5);
                u32 sgn = 0;
                if (comp < 0)
                {
                    sgn = 0x8000u;
                    comp = -comp;
                }
                c[ch] = (sgn | (u32)comp) & 0xffffu;
            }
            else
                c[ch] = (u32)((comp * 31) >> 6) & 0xffffu;
        }
        dst[px] = make_uint2(c[0] | (c[1] << 16), c[2] | 0x3c000000u);
    }
}

// ReconstructLDRPrecise (reference IndexSelector.h:102-112): weights by the reference's linear index
__device__ __forceinline__ int lerp256(int e0, int e1, int w) { return ((256 - w) * e0 + w * e1 + 128) >> 8; }
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int bitsOf(u64 w, int shift, int n) { return (int)((w >> shift) & ((1ull << n) - 1ull)); }

// BC1-BC3 colour: lo = c0 | c1 << 16, hi = the 2-bit indexes.  BC2 / BC3 colour is always four-colour.
__device__ __forceinline__ void bc1Colour(u32 lo, u32 hi, bool fourOnly, int px[16][4])
{
    const int c0 = (int)(lo & 0xffffu), c1 = (int)(lo >> 16);
    int e0[3], e1[3];
    {
        const int r0 = (c0 >> 11) & 31, g0 = (c0 >> 5) & 63, b0 = c0 & 31, r1 = (c1 >> 11) & 31, g1 = (c1 >> 5) & 63, b1 = c1 & 31;
        e0[0] = (r0 << 3) | (r0 >> 2); e0[1] = (g0 << 2) | (g0 >> 4); e0[2] = (b0 << 3) | (b0 >> 2); // S3TC.cpp:52-62
        e1[0] = (r1 << 3) | (r1 >> 2); e1[1] = (g1 << 2) | (g1 >> 4); e1[2] = (b1 << 3) | (b1 >> 2);
    }
    const bool four = fourOnly || c0 > c1;
#pragma unroll
    for (int p = 0; p < 16; p++)
    {
        const int i = (int)((hi >> (2 * p)) & 3u);
        // file index -> weight: four colours 0 / 256 / 85 / 171, three colours 0 / 256 / 128 (+ index 3 transparent)
        const int w = four ? (i == 0 ? 0 : i == 1 ? 256 : i == 2 ? 85 : 171) : (i == 0 ? 0 : i == 1 ? 256 : 128);
        const bool transparent = !four && i == 3;
#pragma unroll
        for (int c = 0; c < 3; c++)
            px[p][c] = transparent ? 0 : lerp256(e0[c], e1[c], w);
        px[p][3] = transparent ? 0 : 255;
    }
}

// BC3 alpha / BC4 / BC5 channel (PackInterpolatedAlpha, S3TC.cpp:343-715): 64-bit little-endian block -> 0..255, or
// -127..127 signed (endpoints read as int8, -128 as -127, ramps in the biased domain 0..254 of Util::BiasSignedInput)
template <bool SIGNED>
__device__ __forceinline__ void interpAlpha(u64 a, int out[16])
{
    int e0, e1;
    bool full;
    if (SIGNED)
    {
        const int r0 = (int)(signed char)(a & 0xffu), r1 = (int)(signed char)((a >> 8) & 0xffu);
        full = r0 > r1;
        e0 = (r0 < -127 ? -127 : r0) + 127;
        e1 = (r1 < -127 ? -127 : r1) + 127;
    }
    else
    {
        e0 = (int)(a & 0xffu);
        e1 = (int)((a >> 8) & 0xffu);
        full = e0 > e1;
    }
    const int high = SIGNED ? 254 : 255;
#pragma unroll
    for (int p = 0; p < 16; p++)
    {
        const int i = (int)((a >> (16 + 3 * p)) & 7u);
        int v;
        if (full)
        {
            const int k = i == 0 ? 0 : i == 1 ? 7 : i - 1; // weights (4681 k + 64) >> 7
            const int w = k == 0 ? 0 : k == 1 ? 37 : k == 2 ? 73 : k == 3 ? 110 : k == 4 ? 146 : k == 5 ? 183 : k == 6 ? 219 : 256;
            v = lerp256(e0, e1, w);
        }
        else
        {
            const int k = i == 0 ? 0 : i == 1 ? 5 : i - 1; // weights (6554 k + 64) >> 7
            const int w = k == 0 ? 0 : k == 1 ? 51 : k == 2 ? 102 : k == 3 ? 154 : k == 4 ? 205 : 256;
            v = i == 6 ? 0 : i == 7 ? high : lerp256(e0, e1, w);
        }
        out[p] = SIGNED ? v - 127 : v;
    }
}

// ETC1 / ETC2 RGB / ETC2 punch-through colour block, w = the block's 8 bytes as a big-endian word.  Texel p = 4 y + x
// takes its index from bit 4 x + y (and 16 + 4 x + y).  ETC1 decodes with the ETC2 rules (its encoder never overflows).
template <bool PT>
__device__ __forceinline__ void etcColour(u64 w, const CvttDeviceTables *__restrict__ T, int px[16][4])
{
    const bool diffBit = ((w >> 33) & 1u) != 0, flip = ((w >> 32) & 1u) != 0;
    const bool differential = PT || diffBit, opaque = !PT || diffBit;
    const int rb = bitsOf(w, 59, 5), gb = bitsOf(w, 51, 5), bb = bitsOf(w, 43, 5);
    const int dr = bitsOf(w, 56, 3), dg = bitsOf(w, 48, 3), db = bitsOf(w, 40, 3);
    const int r2 = rb + (dr >= 4 ? dr - 8 : dr), g2 = gb + (dg >= 4 ? dg - 8 : dg), b2 = bb + (db >= 4 ? db - 8 : db);
    const int mode = !differential ? 0 : (r2 < 0 || r2 > 31) ? 1 : (g2 < 0 || g2 > 31) ? 2 : (b2 < 0 || b2 > 31) ? 3 : 0;
    if (mode == 3)
    {
        // planar: O, H, V in 6/7/6 bits, (x (H - O) + y (V - O) + 4 O + 2) >> 2
        const int ro = bitsOf(w, 57, 6), go = (bitsOf(w, 56, 1) << 6) | bitsOf(w, 49, 6);
        const int bo = (bitsOf(w, 48, 1) << 5) | (bitsOf(w, 43, 2) << 3) | bitsOf(w, 39, 3);
        const int rh = (bitsOf(w, 34, 5) << 1) | bitsOf(w, 32, 1), gh = bitsOf(w, 25, 7), bh = bitsOf(w, 19, 6);
        const int rv = bitsOf(w, 13, 6), gv = bitsOf(w, 6, 7), bv = bitsOf(w, 0, 6);
        const int O[3] = {(ro << 2) | (ro >> 4), (go << 1) | (go >> 6), (bo << 2) | (bo >> 4)};
        const int H[3] = {(rh << 2) | (rh >> 4), (gh << 1) | (gh >> 6), (bh << 2) | (bh >> 4)};
        const int V[3] = {(rv << 2) | (rv >> 4), (gv << 1) | (gv >> 6), (bv << 2) | (bv >> 4)};
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            const int x = p & 3, y = p >> 2;
#pragma unroll
            for (int c = 0; c < 3; c++)
                px[p][c] = clamp255((x * (H[c] - O[c]) + y * (V[c] - O[c]) + 4 * O[c] + 2) >> 2);
            px[p][3] = 255;
        }
        return;
    }
    int paint[4][3];
    int base[2][3];
    int tab[2];
    if (mode == 1)
    {
        const int c1[3] = {((bitsOf(w, 59, 2) << 2) | bitsOf(w, 56, 2)) * 17, bitsOf(w, 52, 4) * 17, bitsOf(w, 48, 4) * 17};
        const int c2[3] = {bitsOf(w, 44, 4) * 17, bitsOf(w, 40, 4) * 17, bitsOf(w, 36, 4) * 17};
        const int d = T->thDistance[(bitsOf(w, 34, 2) << 1) | bitsOf(w, 32, 1)];
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            paint[0][c] = c1[c];
            paint[1][c] = clamp255(c2[c] + d);
            paint[2][c] = c2[c];
            paint[3][c] = clamp255(c2[c] - d);
        }
    }
    else if (mode == 2)
    {
        const int h1[3] = {bitsOf(w, 59, 4), (bitsOf(w, 56, 3) << 1) | bitsOf(w, 52, 1), (bitsOf(w, 51, 1) << 3) | bitsOf(w, 47, 3)};
        const int h2[3] = {bitsOf(w, 43, 4), bitsOf(w, 39, 4), bitsOf(w, 35, 4)};
        const int v1 = (h1[0] << 8) | (h1[1] << 4) | h1[2], v2 = (h2[0] << 8) | (h2[1] << 4) | h2[2];
        const int d = T->thDistance[(bitsOf(w, 34, 1) << 2) | (bitsOf(w, 32, 1) << 1) | (v1 >= v2 ? 1 : 0)];
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            paint[0][c] = clamp255(h1[c] * 17 + d);
            paint[1][c] = clamp255(h1[c] * 17 - d);
            paint[2][c] = clamp255(h2[c] * 17 + d);
            paint[3][c] = clamp255(h2[c] * 17 - d);
        }
    }
    else
    {
        const int sh1[3] = {60, 52, 44}, sh2[3] = {56, 48, 40};
        const int b5[3] = {rb, gb, bb}, s5[3] = {r2, g2, b2};
#pragma unroll
        for (int c = 0; c < 3; c++)
        {
            if (differential)
            {
                base[0][c] = (b5[c] << 3) | (b5[c] >> 2);
                base[1][c] = (s5[c] << 3) | (s5[c] >> 2);
            }
            else
            {
                base[0][c] = bitsOf(w, sh1[c], 4) * 17;
                base[1][c] = bitsOf(w, sh2[c], 4) * 17;
            }
        }
        tab[0] = bitsOf(w, 37, 3);
        tab[1] = bitsOf(w, 34, 3);
    }
#pragma unroll
    for (int p = 0; p < 16; p++)
    {
        const int x = p & 3, y = p >> 2, slot = 4 * x + y;
        const int idx = (bitsOf(w, 16 + slot, 1) << 1) | bitsOf(w, slot, 1);
        int rgb[3];
        if (mode == 0)
        {
            const int sub = (flip ? y : x) >= 2 ? 1 : 0;
            const int t = sub ? tab[1] : tab[0];
            // etc1Modifiers[t] = {-large, -small, +small, +large}; index 0 +small, 1 +large, 2 -small, 3 -large
            int mod = T->etc1Modifiers[t][idx == 0 ? 2 : idx == 1 ? 3 : idx == 2 ? 1 : 0];
            mod = (!opaque && idx == 0) ? 0 : mod;
#pragma unroll
            for (int c = 0; c < 3; c++)
                rgb[c] = clamp255((sub ? base[1][c] : base[0][c]) + mod);
        }
        else
        {
#pragma unroll
            for (int c = 0; c < 3; c++)
                rgb[c] = idx == 0 ? paint[0][c] : idx == 1 ? paint[1][c] : idx == 2 ? paint[2][c] : paint[3][c];
        }
        const bool transparent = !opaque && idx == 2;
#pragma unroll
        for (int c = 0; c < 3; c++)
            px[p][c] = transparent ? 0 : rgb[c];
        px[p][3] = transparent ? 0 : 255;
    }
}

// EAC (big-endian word): KIND 0 = 8-bit alpha 0..255, 1 = R11 unsigned 0..2047, 2 = R11 signed -1023..1023
// (QuantizeETC2Alpha, reference ETC.cpp:2366-2404: base + modifier x multiplier; 11 bits: base 8 b + 4 / 8 b, multiplier 8 m,
// or 1 when m = 0)
template <int KIND>
__device__ __forceinline__ void eacBlock(u64 w, const CvttDeviceTables *__restrict__ T, int out[16])
{
    const int base = bitsOf(w, 56, 8), mult = bitsOf(w, 52, 4), table = bitsOf(w, 48, 4);
    const u32 pos = T->eacPosWord[table];
#pragma unroll
    for (int p = 0; p < 16; p++)
    {
        const int slot = 4 * (p & 3) + (p >> 2);
        const int i = bitsOf(w, 45 - 3 * slot, 3);
        const int pv = (int)((pos >> (8 * (i & 3))) & 0xffu);
        const int mod = i >= 4 ? pv : -pv - 1;
        int v;
        if (KIND == 0)
            v = clamp255(base + mod * mult);
        else if (KIND == 1)
        {
            v = base * 8 + 4 + (mult == 0 ? mod : mod * mult * 8);
            v = v < 0 ? 0 : (v > 2047 ? 2047 : v);
        }
        else
        {
            int sb = base >= 128 ? base - 256 : base;
            sb = sb < -127 ? -127 : sb;
            v = sb * 8 + (mult == 0 ? mod : mod * mult * 8);
            v = v < -1023 ? -1023 : (v > 1023 ? 1023 : v);
        }
        out[p] = v;
    }
}

__device__ __forceinline__ u64 bigEndian64(u32 lo, u32 hi) { return ((u64)__builtin_bswap32(lo) << 32) | (u64)__builtin_bswap32(hi); }

// One packed block (raw: its 8 or 16 bytes as little-endian words) -> px[16][4]: 8-bit formats as 0..255 (BC4S / BC5S
// -127..127), R11 in px[p][0], BC6H the half bit patterns.
template <int F>
__device__ __forceinline__ void decodeTexels(const uint4 raw, const CvttDeviceTables *__restrict__ T, int px[16][4])
{
    if (F == CVTTMI_FMT_BC7)
    {
        u32 pixels[16];
        bc7Block(raw, T, pixels);
#pragma unroll
        for (int p = 0; p < 16; p++)
#pragma unroll
            for (int c = 0; c < 4; c++)
                px[p][c] = (int)((pixels[p] >> (8 * c)) & 0xffu);
    }
    else if (F == CVTTMI_FMT_BC6HU || F == CVTTMI_FMT_BC6HS)
    {
        uint2 t[16];
        bc6hBlock<F == CVTTMI_FMT_BC6HS>(raw, T, t);
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            px[p][0] = (int)(t[p].x & 0xffffu);
            px[p][1] = (int)(t[p].x >> 16);
            px[p][2] = (int)(t[p].y & 0xffffu);
            px[p][3] = 0x3c00;
        }
    }
    else if (F == CVTTMI_FMT_BC1)
        bc1Colour(raw.x, raw.y, false, px);
    else if (F == CVTTMI_FMT_BC2 || F == CVTTMI_FMT_BC3)
    {
        bc1Colour(raw.z, raw.w, true, px);
        if (F == CVTTMI_FMT_BC2)
        {
#pragma unroll
            for (int p = 0; p < 16; p++)
                px[p][3] = (int)(((p < 8 ? raw.x : raw.y) >> (4 * (p & 7))) & 15u) * 17;
        }
        else
        {
            int a[16];
            interpAlpha<false>(((u64)raw.y << 32) | raw.x, a);
#pragma unroll
            for (int p = 0; p < 16; p++)
                px[p][3] = a[p];
        }
    }
    else if (F == CVTTMI_FMT_BC4U || F == CVTTMI_FMT_BC4S || F == CVTTMI_FMT_BC5U || F == CVTTMI_FMT_BC5S)
    {
        constexpr bool sg = F == CVTTMI_FMT_BC4S || F == CVTTMI_FMT_BC5S;
        int r[16], g[16];
        interpAlpha<sg>(((u64)raw.y << 32) | raw.x, r);
        if (F == CVTTMI_FMT_BC5U || F == CVTTMI_FMT_BC5S)
            interpAlpha<sg>(((u64)raw.w << 32) | raw.z, g);
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            px[p][0] = r[p];
            px[p][1] = (F == CVTTMI_FMT_BC5U || F == CVTTMI_FMT_BC5S) ? g[p] : 0;
            px[p][2] = 0;
            px[p][3] = sg ? 127 : 255;
        }
    }
    else if (F == CVTTMI_FMT_ETC1 || F == CVTTMI_FMT_ETC2_RGB)
        etcColour<false>(bigEndian64(raw.x, raw.y), T, px);
    else if (F == CVTTMI_FMT_ETC2_PUNCHTHROUGH)
        etcColour<true>(bigEndian64(raw.x, raw.y), T, px);
    else if (F == CVTTMI_FMT_ETC2_RGBA)
    {
        etcColour<false>(bigEndian64(raw.z, raw.w), T, px);
        int a[16];
        eacBlock<0>(bigEndian64(raw.x, raw.y), T, a);
#pragma unroll
        for (int p = 0; p < 16; p++)
            px[p][3] = a[p];
    }
    else if (F == CVTTMI_FMT_EAC_ALPHA)
    {
        int a[16];
        eacBlock<0>(bigEndian64(raw.x, raw.y), T, a);
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            px[p][0] = px[p][1] = px[p][2] = 0;
            px[p][3] = a[p];
        }
    }
    else
    {
        int v[16];
        eacBlock<F == CVTTMI_FMT_R11U ? 1 : 2>(bigEndian64(raw.x, raw.y), T, v);
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            px[p][0] = v[p];
            px[p][1] = px[p][2] = px[p][3] = 0;
        }
    }
}

template <int F>
__device__ __forceinline__ uint4 loadPacked(const uint8_t *__restrict__ bc, size_t block)
{
    if (Fmt<F>::bcBytes == 8u)
    {
        const uint2 v = *reinterpret_cast<const uint2 *>(bc + block * 8u);
        return make_uint4(v.x, v.y, 0u, 0u);
    }
    return *reinterpret_cast<const uint4 *>(bc + block * 16u);
}
} // namespace
#endif
