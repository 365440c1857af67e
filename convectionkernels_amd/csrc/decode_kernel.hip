// BC7 and BC6H decoders: cvtt::Kernels::DecodeBC7 / DecodeBC6HU / DecodeBC6HS
// (reference ConvectionKernels_API.cpp:288-310 -> BC7Computer::UnpackOne, ConvectionKernels_BC67.cpp:
// 2206-2423, and BC6HComputer::UnpackOne, 3058-3289).  Integer-only, one lane per block: 16 bytes
// in, one PixelBlockU8 (64 B) or PixelBlockF16 (128 B) out; they let quality be checked on the
// device (decode + PSNR) independently of bit-exactness.  Blocks with a reserved mode decode to
// zeros (BC7) / zeros with alpha 1.0 (BC6H), like the reference.
#include "cvtt_kernel_common.h"
#include <hip/hip_fp16.h>
#include <type_traits>
#include "texture_formats.h"

namespace
{
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

__global__ void cvttmi_decode_bc7_kernel(const uint8_t *__restrict__ bc, uint8_t *__restrict__ out, u32 numBlocks,
                                         const CvttDeviceTables *__restrict__ T)
{
    const u32 block = blockIdx.x * blockDim.x + threadIdx.x;
    if (block >= numBlocks)
        return;
    const uint4 raw = *reinterpret_cast<const uint4 *>(bc + (size_t)block * 16u);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)block * 64u);
    u32 pixels[16];
    bc7Block(raw, T, pixels);
    for (int i = 0; i < 4; i++)
        dst[i] = make_uint4(pixels[4 * i], pixels[4 * i + 1], pixels[4 * i + 2], pixels[4 * i + 3]);
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

template <bool SIGNED>
__global__ void cvttmi_decode_bc6h_kernel(const uint8_t *__restrict__ bc, uint8_t *__restrict__ out, u32 numBlocks,
                                          const CvttDeviceTables *__restrict__ T)
{
    const u32 block = blockIdx.x * blockDim.x + threadIdx.x;
    if (block >= numBlocks)
        return;
    const uint4 raw = *reinterpret_cast<const uint4 *>(bc + (size_t)block * 16u);
    uint2 texels[16];
    bc6hBlock<SIGNED>(raw, T, texels);
    uint2 *dst = reinterpret_cast<uint2 *>(out + (size_t)block * 128u);
    for (int px = 0; px < 16; px++)
        dst[px] = texels[px];
}

// ---- every format (include/cvtt_mi355x.h, CVTTMI_FMT_*): texel decoders, the decode kernel, and the measure kernel that
// decodes in registers and adds up the squared error against the source without writing texels to HBM.  Rules and the
// reference lines they follow: INTEGRATION.md, "Decoding and measuring every format"; numpy restatement:
// tests/texture_decode_ref.py. ----
enum
{
    kBC7 = 0, kBC1 = 1, kBC6HU = 2, kBC6HS = 3, kETC2 = 4, kETC2RGBA = 5, kBC2 = 6, kBC3 = 7, kBC4U = 8, kBC4S = 9, kBC5U = 10,
    kBC5S = 11, kETC1 = 12, kETC2PT = 13, kEAC = 14, kR11U = 15, kR11S = 16
};
template <int F> struct Fmt
{
    static constexpr bool hdr = F == kBC6HU || F == kBC6HS;
    static constexpr bool r11 = F == kR11U || F == kR11S;
    static constexpr bool snorm = F == kBC4S || F == kBC5S;
    static constexpr u32 bcBytes = kCvttTextureFormats[F].bcBytes;
    static constexpr u32 mask = kCvttTextureFormats[F].mask;
};
static_assert(kCvttTextureFormatCount == kR11S + 1 && kCvttTextureFormats[kR11U].texBytes == 32 && kCvttTextureFormats[kBC6HU].texBytes == 128,
              "texture_formats.h and the format ids");

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
    if (F == kBC7)
    {
        u32 pixels[16];
        bc7Block(raw, T, pixels);
#pragma unroll
        for (int p = 0; p < 16; p++)
#pragma unroll
            for (int c = 0; c < 4; c++)
                px[p][c] = (int)((pixels[p] >> (8 * c)) & 0xffu);
    }
    else if (F == kBC6HU || F == kBC6HS)
    {
        uint2 t[16];
        bc6hBlock<F == kBC6HS>(raw, T, t);
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            px[p][0] = (int)(t[p].x & 0xffffu);
            px[p][1] = (int)(t[p].x >> 16);
            px[p][2] = (int)(t[p].y & 0xffffu);
            px[p][3] = 0x3c00;
        }
    }
    else if (F == kBC1)
        bc1Colour(raw.x, raw.y, false, px);
    else if (F == kBC2 || F == kBC3)
    {
        bc1Colour(raw.z, raw.w, true, px);
        if (F == kBC2)
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
    else if (F == kBC4U || F == kBC4S || F == kBC5U || F == kBC5S)
    {
        constexpr bool sg = F == kBC4S || F == kBC5S;
        int r[16], g[16];
        interpAlpha<sg>(((u64)raw.y << 32) | raw.x, r);
        if (F == kBC5U || F == kBC5S)
            interpAlpha<sg>(((u64)raw.w << 32) | raw.z, g);
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            px[p][0] = r[p];
            px[p][1] = (F == kBC5U || F == kBC5S) ? g[p] : 0;
            px[p][2] = 0;
            px[p][3] = sg ? 127 : 255;
        }
    }
    else if (F == kETC1 || F == kETC2)
        etcColour<false>(bigEndian64(raw.x, raw.y), T, px);
    else if (F == kETC2PT)
        etcColour<true>(bigEndian64(raw.x, raw.y), T, px);
    else if (F == kETC2RGBA)
    {
        etcColour<false>(bigEndian64(raw.z, raw.w), T, px);
        int a[16];
        eacBlock<0>(bigEndian64(raw.x, raw.y), T, a);
#pragma unroll
        for (int p = 0; p < 16; p++)
            px[p][3] = a[p];
    }
    else if (F == kEAC)
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
        eacBlock<F == kR11U ? 1 : 2>(bigEndian64(raw.x, raw.y), T, v);
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

// (BC7 and BC6H decode through the kernels above)
template <int F>
__global__ __launch_bounds__(256) void cvttmi_decode_kernel(const uint8_t *__restrict__ bc, uint8_t *__restrict__ out, u32 numBlocks,
                                                          const CvttDeviceTables *__restrict__ T)
{
    static_assert(!Fmt<F>::hdr && F != kBC7, "BC7 / BC6H: cvttmi_launch_decode");
    const u32 block = blockIdx.x * blockDim.x + threadIdx.x;
    if (block >= numBlocks)
        return;
    int px[16][4];
    decodeTexels<F>(loadPacked<F>(bc, block), T, px);
    if (Fmt<F>::r11)
    {
        uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)block * 32u);
        u32 h[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            h[i] = ((u32)px[2 * i][0] & 0xffffu) | (((u32)px[2 * i + 1][0] & 0xffffu) << 16);
        dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
        dst[1] = make_uint4(h[4], h[5], h[6], h[7]);
    }
    else
    {
        uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)block * 64u);
        u32 q[16];
#pragma unroll
        for (int p = 0; p < 16; p++)
            q[p] = ((u32)px[p][0] & 0xffu) | (((u32)px[p][1] & 0xffu) << 8) | (((u32)px[p][2] & 0xffu) << 16) | (((u32)px[p][3] & 0xffu) << 24);
#pragma unroll
        for (int i = 0; i < 4; i++)
            dst[i] = make_uint4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
    }
}

// ---- packed blocks -> a linear image (cvttmi_decode_image_device / cvttmi_decode_mips_device).  One lane decodes one block
// and stores its four texel rows; the lanes of a wave hold horizontally adjacent blocks, so one store instruction of a wave
// covers one contiguous run of an image row.  Interior blocks of an image whose base and pitch are multiples of 16 store a
// row as 16 bytes (RGBA8) or 2 x 16 bytes (RGBA16F); a block cut by the right or bottom edge, and every block of an image
// that is not so aligned, stores the texels inside width x height one by one.  Nothing else is written. ----
struct DecodeTarget
{
    uint8_t *image;
    size_t pitch;
    u32 width, height;
};

// block (bx, by) of the image: bx < ceil(width / 4), by < ceil(height / 4)
template <int F>
__device__ __forceinline__ void storeBlockTexels(const int px[16][4], const DecodeTarget &t, u32 bx, u32 by)
{
    constexpr u32 kWords = Fmt<F>::hdr ? 2u : 1u; // 32-bit words of a texel
    u32 w[16][kWords];
#pragma unroll
    for (int p = 0; p < 16; p++)
    {
        if (Fmt<F>::hdr)
        {
            w[p][0] = ((u32)px[p][0] & 0xffffu) | (((u32)px[p][1] & 0xffffu) << 16);
            w[p][kWords - 1] = ((u32)px[p][2] & 0xffffu) | (((u32)px[p][3] & 0xffffu) << 16);
        }
        else
            w[p][0] = ((u32)px[p][0] & 0xffu) | (((u32)px[p][1] & 0xffu) << 8) | (((u32)px[p][2] & 0xffu) << 16) | (((u32)px[p][3] & 0xffu) << 24);
    }
    const u32 x0 = bx * 4u, y0 = by * 4u;
    const u32 cols = t.width - x0 < 4u ? t.width - x0 : 4u, rows = t.height - y0 < 4u ? t.height - y0 : 4u;
    uint8_t *dst = t.image + (size_t)y0 * t.pitch + (size_t)x0 * (4u * kWords);
    const bool wide = ((reinterpret_cast<uintptr_t>(t.image) | t.pitch) & 15u) == 0;
    if (wide && cols == 4u && rows == 4u)
    {
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            uint4 *row = reinterpret_cast<uint4 *>(dst + (size_t)r * t.pitch);
            if (Fmt<F>::hdr)
            {
                row[0] = make_uint4(w[4 * r][0], w[4 * r][kWords - 1], w[4 * r + 1][0], w[4 * r + 1][kWords - 1]);
                row[1] = make_uint4(w[4 * r + 2][0], w[4 * r + 2][kWords - 1], w[4 * r + 3][0], w[4 * r + 3][kWords - 1]);
            }
            else
                row[0] = make_uint4(w[4 * r][0], w[4 * r + 1][0], w[4 * r + 2][0], w[4 * r + 3][0]);
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++)
            if ((u32)r < rows && (u32)c < cols)
            {
                uint8_t *texel = dst + (size_t)r * t.pitch + (size_t)c * (4u * kWords);
                if (Fmt<F>::hdr)
                    *reinterpret_cast<uint2 *>(texel) = make_uint2(w[4 * r + c][0], w[4 * r + c][kWords - 1]);
                else
                    *reinterpret_cast<u32 *>(texel) = w[4 * r + c][0];
            }
}

constexpr u32 kImageWG = 256; // lanes of a workgroup = blocks of one block row

// grid: x over the block columns (kImageWG per workgroup), y and z over the block rows (y alone is limited to 65 535), so
// no lane divides.  bc: the blocksPerRow x blockRows blocks, row-major.
template <int F>
__global__ __launch_bounds__(256) void cvttmi_decode_image_kernel(const uint8_t *__restrict__ bc, const DecodeTarget img, u32 blocksPerRow,
                                                                u32 blockRows, const CvttDeviceTables *__restrict__ T)
{
    const u32 bx = blockIdx.x * kImageWG + threadIdx.x;
    const u32 by = blockIdx.z * gridDim.y + blockIdx.y;
    if (bx >= blocksPerRow || by >= blockRows)
        return;
    int px[16][4];
    decodeTexels<F>(loadPacked<F>(bc, (size_t)by * blocksPerRow + bx), T, px);
    storeBlockTexels<F>(px, img, bx, by);
}

// A whole mip chain in one launch: the levels' blocks are consecutive in bc, so a lane's global block index is also its
// block's place in bc; its level is the last one whose firstBlock is not above that index (the table is in level order).
template <int F>
__global__ __launch_bounds__(256) void cvttmi_decode_mips_kernel(const uint8_t *__restrict__ bc, const CvttDecodeLevels levels,
                                                               const CvttDeviceTables *__restrict__ T)
{
    const u32 block = blockIdx.x * kImageWG + threadIdx.x;
    if (block >= levels.numBlocks)
        return;
    u32 l = 0;
    for (u32 i = 1; i < levels.count; i++)
        l = block >= levels.level[i].firstBlock ? i : l;
    const CvttDecodeLevel &L = levels.level[l];
    DecodeTarget img;
    img.image = L.image;
    img.pitch = L.pitch;
    img.width = L.width;
    img.height = L.height;
    const u32 local = block - L.firstBlock, by = local / L.blocksPerRow;
    int px[16][4];
    decodeTexels<F>(loadPacked<F>(bc, block), T, px);
    storeBlockTexels<F>(px, img, local - by * L.blocksPerRow, by);
}

// half bits -> float (exact)
__device__ __forceinline__ float halfToFloat(int bits) { return __half2float(__ushort_as_half((unsigned short)(bits & 0xffff))); }

// The source texels of one block as the encoder reads them.  SRC 0: the encoder's input blocks; 1: a linear RGBA8 image;
// 2: a linear RGBA16F image (texels outside width x height are flagged invalid and count nowhere).
struct MeasureImage
{
    const uint8_t *image;
    size_t pitch;
    u32 width, height, blocksPerRow;
    size_t firstBlock; // image block of the launch's block 0
};

template <int F>
__device__ __forceinline__ int sourceValue(u32 word, int c)
{
    // 8-bit sources: BC4S / BC5S read int8 with -128 as -127 (Util::BiasSignedInput)
    const int b = (int)((word >> (8 * c)) & 0xffu);
    if (Fmt<F>::snorm)
    {
        const int s = b >= 128 ? b - 256 : b;
        return s < -127 ? -127 : s;
    }
    return b;
}

constexpr u32 kMeasureWG = 256;
constexpr u32 kTotalWG = 1024; // lanes of the one-workgroup total
constexpr u32 kMeasureLaunch = 1u << 24; // blocks per launch: the slab holds kMeasureLaunch / kMeasureWG partials

template <int F, int SRC>
__global__ __launch_bounds__(256) void cvttmi_measure_kernel(const uint8_t *__restrict__ bc, const uint8_t *__restrict__ source,
                                                           const MeasureImage img, u32 numBlocks, void *__restrict__ blockError,
                                                           void *__restrict__ slab, const CvttDeviceTables *__restrict__ T)
{
    typedef typename std::conditional<Fmt<F>::hdr, double, u64>::type Acc;
    __shared__ Acc part[4][kMeasureWG];
    const u32 tid = threadIdx.x;
    const u32 block = blockIdx.x * kMeasureWG + tid;
    Acc ch[4] = {0, 0, 0, 0};
    if (block < numBlocks)
    {
        int px[16][4];
        decodeTexels<F>(loadPacked<F>(bc, block), T, px);
        u32 valid = 0xffffu;
        if (Fmt<F>::hdr)
        {
            // float per block: texel 0..15, channel 0..2 inside; per channel: texel 0..15
            float src[16][3];
            if (SRC == 0)
            {
                const uint2 *s = reinterpret_cast<const uint2 *>(source + (size_t)block * 128u);
#pragma unroll
                for (int p = 0; p < 16; p++)
                {
                    const uint2 v = s[p];
                    src[p][0] = halfToFloat((int)(v.x & 0xffffu));
                    src[p][1] = halfToFloat((int)(v.x >> 16));
                    src[p][2] = halfToFloat((int)(v.y & 0xffffu));
                }
            }
            else
            {
                const size_t ib = img.firstBlock + block;
                const u32 bx = (u32)(ib % img.blocksPerRow), by = (u32)(ib / img.blocksPerRow);
                valid = 0;
#pragma unroll
                for (int p = 0; p < 16; p++)
                {
                    const u32 x = bx * 4u + (u32)(p & 3), y = by * 4u + (u32)(p >> 2);
                    uint2 v = make_uint2(0u, 0u);
                    if (x < img.width && y < img.height)
                    {
                        v = *reinterpret_cast<const uint2 *>(img.image + (size_t)y * img.pitch + (size_t)x * 8u);
                        valid |= 1u << p;
                    }
                    src[p][0] = halfToFloat((int)(v.x & 0xffffu));
                    src[p][1] = halfToFloat((int)(v.x >> 16));
                    src[p][2] = halfToFloat((int)(v.y & 0xffffu));
                }
            }
            float total = 0.0f, per[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int p = 0; p < 16; p++)
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    const float d = halfToFloat(px[p][c]) - src[p][c];
                    const float sq = ((valid >> p) & 1u) ? d * d : 0.0f;
                    total = total + sq;
                    per[c] = per[c] + sq;
                }
            if (blockError)
                static_cast<float *>(blockError)[block] = total;
#pragma unroll
            for (int c = 0; c < 3; c++)
                ch[c] = (Acc)per[c];
        }
        else
        {
            int src[16][4];
            if (SRC == 0 && Fmt<F>::r11)
            {
                const uint4 *s = reinterpret_cast<const uint4 *>(source + (size_t)block * 32u);
                const uint4 a = s[0], b = s[1];
                const u32 wds[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int p = 0; p < 16; p++)
                {
                    int v = (int)(short)((wds[p >> 1] >> (16 * (p & 1))) & 0xffffu);
                    // the encoder's clamp (reference ETC.cpp:2087-2113)
                    if (F == kR11U)
                        v = v < 0 ? 0 : (v > 2047 ? 2047 : v);
                    else
                        v = v < -1023 ? -1023 : (v > 1023 ? 1023 : v);
                    src[p][0] = v;
                    src[p][1] = src[p][2] = src[p][3] = 0;
                }
            }
            else if (SRC == 0)
            {
                const uint4 *s = reinterpret_cast<const uint4 *>(source + (size_t)block * 64u);
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const uint4 v = s[i];
                    const u32 wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int c = 0; c < 4; c++)
                            src[4 * i + j][c] = sourceValue<F>(wds[j], c);
                }
            }
            else
            {
                const size_t ib = img.firstBlock + block;
                const u32 bx = (u32)(ib % img.blocksPerRow), by = (u32)(ib / img.blocksPerRow);
                valid = 0;
#pragma unroll
                for (int p = 0; p < 16; p++)
                {
                    const u32 x = bx * 4u + (u32)(p & 3), y = by * 4u + (u32)(p >> 2);
                    u32 v = 0;
                    if (x < img.width && y < img.height)
                    {
                        v = *reinterpret_cast<const u32 *>(img.image + (size_t)y * img.pitch + (size_t)x * 4u);
                        valid |= 1u << p;
                    }
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        src[p][c] = sourceValue<F>(v, c);
                }
            }
            u32 per[4] = {0, 0, 0, 0};
#pragma unroll
            for (int p = 0; p < 16; p++)
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if ((Fmt<F>::mask >> c) & 1u)
                    {
                        const int d = px[p][c] - src[p][c];
                        per[c] += ((valid >> p) & 1u) ? (u32)(d * d) : 0u;
                    }
            if (blockError)
                static_cast<u32 *>(blockError)[block] = per[0] + per[1] + per[2] + per[3];
#pragma unroll
            for (int c = 0; c < 4; c++)
                ch[c] = (Acc)per[c];
        }
    }
    // one partial per workgroup: halving tree in LDS (the order cvtt_mi355x.h documents)
#pragma unroll
    for (int c = 0; c < 4; c++)
        part[c][tid] = ch[c];
    __syncthreads();
    for (u32 s = kMeasureWG / 2; s > 0; s >>= 1)
    {
        if (tid < s)
#pragma unroll
            for (int c = 0; c < 4; c++)
                part[c][tid] = part[c][tid] + part[c][tid + s];
        __syncthreads();
    }
    if (tid < 4)
        static_cast<Acc *>(slab)[(size_t)blockIdx.x * 4u + tid] = part[tid][0];
}

// One workgroup of 1024 lanes: lane t adds the partials t, t + 1024, t + 2048, ... of a launch in that order (the loads of
// eight of them are issued before their adds: with one dependent load per trip, 65 536 partials took 100 us), then a halving
// tree in LDS as above, then into the totals (accumulate: added to what the previous launch of the call wrote).
template <bool HDR>
__global__ __launch_bounds__(1024) void cvttmi_measure_total_kernel(const void *__restrict__ slab, u32 numPartials, cvttmi_error_totals *totals,
                                                                  int accumulate, u64 texels, u32 mask, int format)
{
    typedef typename std::conditional<HDR, double, u64>::type Acc;
    __shared__ Acc part[4][kTotalWG];
    const u32 tid = threadIdx.x;
    const Acc *p = static_cast<const Acc *>(slab);
    Acc acc[4] = {0, 0, 0, 0};
    constexpr u32 kRows = 8;
    for (u32 base = tid; base < numPartials; base += kRows * kTotalWG)
    {
        Acc v[kRows][4];
#pragma unroll
        for (u32 r = 0; r < kRows; r++)
        {
            const u32 i = base + r * kTotalWG;
#pragma unroll
            for (int c = 0; c < 4; c++)
                v[r][c] = i < numPartials ? p[(size_t)i * 4u + c] : (Acc)0; // (adding 0 leaves a sum of non-negative terms as it is)
        }
#pragma unroll
        for (u32 r = 0; r < kRows; r++)
#pragma unroll
            for (int c = 0; c < 4; c++)
                acc[c] = acc[c] + v[r][c];
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
        part[c][tid] = acc[c];
    __syncthreads();
    for (u32 s = kTotalWG / 2; s > 0; s >>= 1)
    {
        if (tid < s)
#pragma unroll
            for (int c = 0; c < 4; c++)
                part[c][tid] = part[c][tid] + part[c][tid + s];
        __syncthreads();
    }
    if (tid == 0)
    {
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
            const Acc v = ((mask >> c) & 1u) ? part[c][0] : (Acc)0;
            if (HDR)
            {
                totals->sse[c] = 0;
                totals->sseHdr[c] = (accumulate ? totals->sseHdr[c] : 0.0) + (double)v;
            }
            else
            {
                totals->sse[c] = (accumulate ? totals->sse[c] : 0ull) + (u64)v;
                totals->sseHdr[c] = 0.0;
            }
        }
        totals->texels = (accumulate ? totals->texels : 0ull) + texels;
        totals->channelMask = mask;
        totals->format = format;
    }
}

template <int F>
hipError_t launchDecodeFormat(const void *d_bc, void *d_out, u32 numBlocks, const CvttDeviceTables *T, hipStream_t stream)
{
    hipLaunchKernelGGL(cvttmi_decode_kernel<F>, dim3((numBlocks + 255u) / 256u), dim3(256), 0, stream, (const uint8_t *)d_bc, (uint8_t *)d_out,
                       numBlocks, T);
    return hipGetLastError();
}

template <int F>
hipError_t launchDecodeImage(const void *d_bc, const DecodeTarget &img, const CvttDeviceTables *T, hipStream_t stream)
{
    const u32 blocksPerRow = (u32)(((u64)img.width + 3u) / 4u), blockRows = (u32)(((u64)img.height + 3u) / 4u);
    const u32 gy = blockRows < 65535u ? blockRows : 65535u;
    hipLaunchKernelGGL(cvttmi_decode_image_kernel<F>, dim3((blocksPerRow + kImageWG - 1u) / kImageWG, gy, (blockRows + gy - 1u) / gy), dim3(kImageWG),
                       0, stream, (const uint8_t *)d_bc, img, blocksPerRow, blockRows, T);
    return hipGetLastError();
}

template <int F>
hipError_t launchDecodeMips(const void *d_bc, const CvttDecodeLevels &levels, const CvttDeviceTables *T, hipStream_t stream)
{
    hipLaunchKernelGGL(cvttmi_decode_mips_kernel<F>, dim3((u32)(((u64)levels.numBlocks + kImageWG - 1u) / kImageWG)), dim3(kImageWG), 0, stream,
                       (const uint8_t *)d_bc, levels, T);
    return hipGetLastError();
}

template <int F, int SRC>
hipError_t launchMeasureFormat(const void *d_bc, const void *d_source, const MeasureImage &img, u32 numBlocks, void *d_blockError,
                               void *d_slab, cvttmi_error_totals *d_totals, int accumulate, u64 texels, const CvttDeviceTables *T,
                               hipStream_t stream)
{
    const u32 groups = (numBlocks + kMeasureWG - 1u) / kMeasureWG;
    if (groups)
    {
        hipLaunchKernelGGL((cvttmi_measure_kernel<F, SRC>), dim3(groups), dim3(kMeasureWG), 0, stream, (const uint8_t *)d_bc,
                           (const uint8_t *)d_source, img, numBlocks, d_blockError, d_slab, T);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(cvttmi_measure_total_kernel<Fmt<F>::hdr>, dim3(1), dim3(kTotalWG), 0, stream, (const void *)d_slab, groups, d_totals,
                       accumulate, texels, Fmt<F>::mask, F);
    return hipGetLastError();
}

template <int F>
hipError_t measureBySource(int src, const void *d_bc, const void *d_source, const MeasureImage &img, u32 numBlocks, void *d_blockError,
                           void *d_slab, cvttmi_error_totals *d_totals, int accumulate, u64 texels, const CvttDeviceTables *T, hipStream_t stream)
{
    if (src == 0)
        return launchMeasureFormat<F, 0>(d_bc, d_source, img, numBlocks, d_blockError, d_slab, d_totals, accumulate, texels, T, stream);
    // image forms: RGBA16F for BC6H, RGBA8 for every 8-bit format, none for R11 (the shim rejects other pairs)
    constexpr int imageSrc = Fmt<F>::hdr ? 2 : 1;
    if (Fmt<F>::r11 || src != imageSrc)
        return hipErrorInvalidValue;
    return launchMeasureFormat<F, Fmt<F>::r11 ? 0 : imageSrc>(d_bc, d_source, img, numBlocks, d_blockError, d_slab, d_totals, accumulate, texels, T, stream);
}
} // namespace

extern "C" hipError_t cvttmi_launch_decode(const void *d_bc, void *d_out, uint32_t numBlocks, int format,
                                           const CvttDeviceTables *d_tables, hipStream_t stream)
{
    if (numBlocks == 0)
        return hipSuccess;
    const dim3 grid((numBlocks + 63u) / 64u), block(64);
    if (format == 0)
        hipLaunchKernelGGL(cvttmi_decode_bc7_kernel, grid, block, 0, stream, (const uint8_t *)d_bc, (uint8_t *)d_out, numBlocks, d_tables);
    else if (format == 1)
        hipLaunchKernelGGL(cvttmi_decode_bc6h_kernel<false>, grid, block, 0, stream, (const uint8_t *)d_bc, (uint8_t *)d_out, numBlocks, d_tables);
    else
        hipLaunchKernelGGL(cvttmi_decode_bc6h_kernel<true>, grid, block, 0, stream, (const uint8_t *)d_bc, (uint8_t *)d_out, numBlocks, d_tables);
    return hipGetLastError();
}

// every format: 0 .. CVTTMI_FMT_COUNT - 1.  BC7 and BC6H go through the kernels above, so their output stays that of
// cvttmi_decode_bc7 / bc6h byte for byte.
extern "C" hipError_t cvttmi_launch_decode_format(const void *d_bc, void *d_out, uint32_t numBlocks, int format,
                                                  const CvttDeviceTables *d_tables, hipStream_t stream)
{
    switch (format)
    {
    case kBC7: return cvttmi_launch_decode(d_bc, d_out, numBlocks, 0, d_tables, stream);
    case kBC6HU: return cvttmi_launch_decode(d_bc, d_out, numBlocks, 1, d_tables, stream);
    case kBC6HS: return cvttmi_launch_decode(d_bc, d_out, numBlocks, 2, d_tables, stream);
    }
    if (numBlocks == 0)
        return hipSuccess;
    switch (format)
    {
    case kBC1: return launchDecodeFormat<kBC1>(d_bc, d_out, numBlocks, d_tables, stream);
    case kETC2: return launchDecodeFormat<kETC2>(d_bc, d_out, numBlocks, d_tables, stream);
    case kETC2RGBA: return launchDecodeFormat<kETC2RGBA>(d_bc, d_out, numBlocks, d_tables, stream);
    case kBC2: return launchDecodeFormat<kBC2>(d_bc, d_out, numBlocks, d_tables, stream);
    case kBC3: return launchDecodeFormat<kBC3>(d_bc, d_out, numBlocks, d_tables, stream);
    case kBC4U: return launchDecodeFormat<kBC4U>(d_bc, d_out, numBlocks, d_tables, stream);
    case kBC4S: return launchDecodeFormat<kBC4S>(d_bc, d_out, numBlocks, d_tables, stream);
    case kBC5U: return launchDecodeFormat<kBC5U>(d_bc, d_out, numBlocks, d_tables, stream);
    case kBC5S: return launchDecodeFormat<kBC5S>(d_bc, d_out, numBlocks, d_tables, stream);
    case kETC1: return launchDecodeFormat<kETC1>(d_bc, d_out, numBlocks, d_tables, stream);
    case kETC2PT: return launchDecodeFormat<kETC2PT>(d_bc, d_out, numBlocks, d_tables, stream);
    case kEAC: return launchDecodeFormat<kEAC>(d_bc, d_out, numBlocks, d_tables, stream);
    case kR11U: return launchDecodeFormat<kR11U>(d_bc, d_out, numBlocks, d_tables, stream);
    case kR11S: return launchDecodeFormat<kR11S>(d_bc, d_out, numBlocks, d_tables, stream);
    }
    return hipErrorInvalidValue;
}

// One launch of the measure (numBlocks <= 2^24, > 0) and its total: source 0 = blocks, 1 = RGBA8 image, 2 = RGBA16F image
// (image: width, height, pitch, blocks per row = ceil(width / 4); d_bc starts at block firstBlock of the image).  d_slab: (2^24 / 256) x 4 x 8 bytes.
extern "C" hipError_t cvttmi_launch_measure(const void *d_bc, const void *d_source, int source, uint32_t width, uint32_t height,
                                            size_t pitch, size_t firstBlock, uint32_t numBlocks, int format, void *d_blockError, void *d_slab,
                                            cvttmi_error_totals *d_totals, int accumulate, uint64_t texels,
                                            const CvttDeviceTables *d_tables, hipStream_t stream)
{
    if (numBlocks > kMeasureLaunch)
        return hipErrorInvalidValue;
    MeasureImage img;
    img.image = (const uint8_t *)d_source;
    img.pitch = pitch;
    img.width = width;
    img.height = height;
    img.blocksPerRow = (width + 3u) / 4u;
    img.firstBlock = firstBlock;
#define CVTTMI_MEASURE_CASE(F) \
    case F: return measureBySource<F>(source, d_bc, d_source, img, numBlocks, d_blockError, d_slab, d_totals, accumulate, texels, d_tables, stream);
    switch (format)
    {
        CVTTMI_MEASURE_CASE(kBC7) CVTTMI_MEASURE_CASE(kBC1) CVTTMI_MEASURE_CASE(kBC6HU) CVTTMI_MEASURE_CASE(kBC6HS)
        CVTTMI_MEASURE_CASE(kETC2) CVTTMI_MEASURE_CASE(kETC2RGBA) CVTTMI_MEASURE_CASE(kBC2) CVTTMI_MEASURE_CASE(kBC3)
        CVTTMI_MEASURE_CASE(kBC4U) CVTTMI_MEASURE_CASE(kBC4S) CVTTMI_MEASURE_CASE(kBC5U) CVTTMI_MEASURE_CASE(kBC5S)
        CVTTMI_MEASURE_CASE(kETC1) CVTTMI_MEASURE_CASE(kETC2PT) CVTTMI_MEASURE_CASE(kEAC) CVTTMI_MEASURE_CASE(kR11U)
        CVTTMI_MEASURE_CASE(kR11S)
    }
#undef CVTTMI_MEASURE_CASE
    return hipErrorInvalidValue;
}

// Packed blocks -> linear images: every format but R11, which has no image form (the shim rejects it, and the wrong texel
// size for a format, before it comes here).
#define CVTTMI_IMAGE_FORMATS(CASE) \
    CASE(kBC7) CASE(kBC1) CASE(kBC6HU) CASE(kBC6HS) CASE(kETC2) CASE(kETC2RGBA) CASE(kBC2) CASE(kBC3) CASE(kBC4U) CASE(kBC4S) \
    CASE(kBC5U) CASE(kBC5S) CASE(kETC1) CASE(kETC2PT) CASE(kEAC)

// d_bc: the ceil(width / 4) x ceil(height / 4) blocks, row-major (fewer than 2^32); d_image: width x height texels of 4 bytes
// (BC6H: 8), `pitch` bytes between rows
extern "C" hipError_t cvttmi_launch_decode_image(const void *d_bc, void *d_image, size_t pitch, uint32_t width, uint32_t height, int format,
                                                 const CvttDeviceTables *d_tables, hipStream_t stream)
{
    DecodeTarget img;
    img.image = (uint8_t *)d_image;
    img.pitch = pitch;
    img.width = width;
    img.height = height;
#define CVTTMI_DECODE_IMAGE_CASE(F) \
    case F: return launchDecodeImage<F>(d_bc, img, d_tables, stream);
    switch (format)
    {
        CVTTMI_IMAGE_FORMATS(CVTTMI_DECODE_IMAGE_CASE)
    }
#undef CVTTMI_DECODE_IMAGE_CASE
    return hipErrorInvalidValue;
}

// levels->level[0 .. count - 1] in level order, their blocks consecutive in d_bc; 0 < numBlocks < 2^32
extern "C" hipError_t cvttmi_launch_decode_mips(const void *d_bc, const CvttDecodeLevels *levels, int format, const CvttDeviceTables *d_tables,
                                                hipStream_t stream)
{
    if (levels->count == 0 || levels->count > kCvttDecodeLevels || levels->numBlocks == 0)
        return hipErrorInvalidValue;
#define CVTTMI_DECODE_MIPS_CASE(F) \
    case F: return launchDecodeMips<F>(d_bc, *levels, d_tables, stream);
    switch (format)
    {
        CVTTMI_IMAGE_FORMATS(CVTTMI_DECODE_MIPS_CASE)
    }
#undef CVTTMI_DECODE_MIPS_CASE
    return hipErrorInvalidValue;
}
#undef CVTTMI_IMAGE_FORMATS
