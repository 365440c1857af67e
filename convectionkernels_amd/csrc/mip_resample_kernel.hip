// The mip kernels wider than 2x2 (include/cvtt_mi355x.h, "mip chains", CVTTMI_MIP_KERNEL_* and CVTTMI_MIP_WRAP_*): one level per
// launch like the other mip filters, one kernel template for every pixel kind (RGBA8 and RGBA8_SNORM described first, RGBA16F
// at the end).  An output texel reads n x n source texels (n = 4, 8 or
// 12 taps per direction, one Q14 table for every texel: tools/gen_mip_kernels.py), separably:
//   a workgroup of 256 lanes owns a tile of kTileX x kTileY output texels.  Horizontal pass: for each of the 2 kTileY + n - 2
//   source rows under the tile (wrapped), a lane makes four neighbouring h' from one window of n + 6 source texels -- 16-byte
//   reads where the chunk lies inside the row and the row starts allow them, texel reads through the wrap otherwise -- and stores
//   them in LDS.  Vertical pass: a lane makes four output texels of one column from a window of n + 6 LDS entries and writes
//   each with a 4-byte store (a wave writes 256 contiguous bytes of a row).
// The value of a texel's channel is taken in the horizontal pass: the byte (plain, and always channel 3), T[byte] (SRGB) or X
// (NORMAL).  LDS per entry: plain int16 x 4; SRGB int32 x 4; NORMAL int16 x 4 of X and alpha plus int16 x 4 of the plain
// bytes, which the vertical pass reads only where the three sums of X are all zero.  At most 42 x 64 x 16 B + the sRGB tables =
// 48.5 KB a workgroup: three workgroups share a CU.  The taps arrive as kernel arguments (scalar registers).  No scratch.
// Every product is a 24-bit multiply (__mul24: full rate, where a 32-bit multiply runs at a quarter): a tap is below 2^13, a value
// or an h' below 2^17 (sRGB: T <= 65535, |h'| <= 78727), and the generator asserts that the sums stay inside int32.
// RGBA16F (resample_common.h, "RGBA16F"; the plain rule only): the same tile, items and lanes with KIND = kRGBA16F.  A texel is a
// uint2, so a 16-byte read holds two; the window of n + 6 texels starts at an odd column, so one texel leads it from the 16-byte
// boundary.  Taps, sums and entries are floats: an LDS entry is the four float sums (42 x 64 x 16 B at most, as under SRGB, and no
// tables), an output texel an 8-byte store of the sums clamped to [lo, 65504].  No scratch.
#include "resample_common.h"
#include "cvtt_launchers.h"

namespace
{
enum
{
    kTileX = 64,
    kTileY = 16
};

// what the pixel kind decides: the texel, the number type of taps, sums and entries, and one multiply-add
template <int KIND>
struct MipTaps
{
    typename std::conditional<KIND == kRGBA16F, float, int>::type w[12];
};

__device__ __forceinline__ int mulAdd(int acc, int w, int v)
{
    return acc + __mul24(w, v);
}

__device__ __forceinline__ float mulAdd(float acc, float w, float v) // the product and the sum round on their own (-ffp-contract=off)
{
    return acc + w * v;
}

// `lo`: the lower clamp of an RGBA16F texel (the integer kinds do not read it)
template <int KIND, int RULE, int NTAPS>
__global__ void __launch_bounds__(256) cvttmi_mipresample_kernel(const uint8_t *__restrict__ src, size_t srcPitch,
                                                                  uint8_t *__restrict__ dst, size_t dstPitch, uint32_t srcW, uint32_t srcH,
                                                                  uint32_t dstW, uint32_t dstH, size_t srcLayer, size_t dstLayer,
                                                                  uint32_t wrap, uint32_t wide, uint32_t tilesY, MipTaps<KIND> taps, float lo)
{
    constexpr bool kHalf = KIND == kRGBA16F;
    typedef typename std::conditional<kHalf, uint2, uint32_t>::type Texel;
    typedef typename std::conditional<kHalf, float, int>::type Num;
    typedef typename std::conditional<kHalf, float4, typename std::conditional<RULE == kSrgb, int4, short4>::type>::type Entry;
    constexpr int kPer = 16 / sizeof(Texel);      // texels of a 16-byte read
    constexpr int kRows = 2 * kTileY + NTAPS - 2; // source rows under a tile
    constexpr int kWindow = NTAPS + 6;            // source texels (LDS rows) under four neighbouring outputs
    constexpr int kLead = (1 - NTAPS / 2) & (kPer - 1); // texels between the 16-byte boundary and the window's first texel
    constexpr int kChunks = (kLead + kWindow + kPer - 1) / kPer;
    constexpr int kSums = RULE == kNormal ? 7 : 4;
    __shared__ Entry hbuf[kRows * kTileX];
    __shared__ short4 pbuf[RULE == kNormal ? kRows * kTileX : 1]; // NORMAL: the plain h' of channels 0..2
    __shared__ SrgbTables tables;                                 // (no LDS is allocated where it is not read)
    src += blockIdx.z * srcLayer;
    dst += blockIdx.z * dstLayer;
    if (RULE == kSrgb)
    {
        loadSrgbTables(tables, 256u, threadIdx.x);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x;
    const uint32_t x0 = blockIdx.x * kTileX;
    const uint32_t groups = (min(dstW - x0, (uint32_t)kTileX) + 3u) / 4u; // groups of four output columns with a texel in them
    for (uint32_t ty = blockIdx.y; ty < tilesY; ty += gridDim.y)
    {
        const uint32_t y0 = ty * kTileY;
        const uint32_t tileH = min(dstH - y0, (uint32_t)kTileY);
        const uint32_t rows = 2u * tileH + NTAPS - 2u;

        // horizontal pass: item = (source row r of the tile, group g of four output columns)
        for (uint32_t item = lane; item < rows * groups; item += 256u)
        {
            const uint32_t r = item / groups, g = item - r * groups;
            const Walk wy = walkFrom(2 * (int64_t)y0 + 1 - NTAPS / 2 + (int64_t)r, srcH, wrap);
            const uint8_t *row = src + (size_t)walkIndex(wy) * srcPitch;
            const int64_t c0 = 2 * (int64_t)(x0 + 4u * g) + 1 - NTAPS / 2 - kLead; // a multiple of kPer
            Texel texel[kPer * kChunks];
            Walk wx = walkFrom(c0, srcW, wrap);
#pragma unroll
            for (int q = 0; q < kChunks; q++)
            {
                const int64_t c = c0 + kPer * q;
                if (wide && c >= 0 && c + kPer <= (int64_t)srcW)
                {
                    const uint4 v = *reinterpret_cast<const uint4 *>(row + sizeof(Texel) * c);
                    if constexpr (kHalf)
                    {
                        texel[2 * q] = make_uint2(v.x, v.y);
                        texel[2 * q + 1] = make_uint2(v.z, v.w);
                    }
                    else
                    {
                        texel[4 * q] = v.x;
                        texel[4 * q + 1] = v.y;
                        texel[4 * q + 2] = v.z;
                        texel[4 * q + 3] = v.w;
                    }
#pragma unroll
                    for (int e = 0; e < kPer; e++)
                        walkStep(wx); // (inside the row the walk is at c itself, under every wrap)
                }
                else
                {
#pragma unroll
                    for (int e = 0; e < kPer; e++)
                    {
                        texel[kPer * q + e] = reinterpret_cast<const Texel *>(row)[walkIndex(wx)];
                        walkStep(wx);
                    }
                }
            }
            Num h[4][kSums];
#pragma unroll
            for (int c = 0; c < kSums; c++)
            {
                Num v[kWindow];
#pragma unroll
                for (int i = 0; i < kWindow; i++)
                {
                    if constexpr (kHalf)
                        v[i] = halfValue((c < 2 ? texel[kLead + i].x : texel[kLead + i].y) >> (16 * (c & 1)));
                    else
                        v[i] = ruleValue<KIND, RULE>(texel[kLead + i], c, tables.lin);
                }
#pragma unroll
                for (int j = 0; j < 4; j++)
                {
                    Num acc = 0;
#pragma unroll
                    for (int k = 0; k < NTAPS; k++)
                        acc = mulAdd(acc, taps.w[k], v[2 * j + k]);
                    if constexpr (kHalf)
                        h[j][c] = acc;
                    else
                        h[j][c] = (RULE == kSrgb && c < 3) ? (acc + (1 << 13)) >> 14 : (acc + 512) >> 10;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const uint32_t at = r * kTileX + 4u * g + j;
                if constexpr (kHalf)
                    hbuf[at] = make_float4(h[j][0], h[j][1], h[j][2], h[j][3]);
                else if constexpr (RULE == kSrgb)
                    hbuf[at] = make_int4(h[j][0], h[j][1], h[j][2], h[j][3]);
                else
                    hbuf[at] = make_short4((short)h[j][0], (short)h[j][1], (short)h[j][2], (short)h[j][3]);
                if constexpr (RULE == kNormal)
                    pbuf[at] = make_short4((short)h[j][4], (short)h[j][5], (short)h[j][6], 0);
            }
        }
        __syncthreads();

        // vertical pass: lane = (column x of the tile, rows 4 yg .. 4 yg + 3 of the tile)
        const uint32_t x = lane & (kTileX - 1), yg = lane / kTileX;
        if (x0 + x < dstW && 4u * yg < tileH)
        {
            Num s[4][4];
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int c = 0; c < 4; c++)
                    s[j][c] = 0;
#pragma unroll
            for (int i = 0; i < kWindow; i++)
            {
                const Entry e = hbuf[(8u * yg + i) * kTileX + x];
                const Num ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (i - 2 * j >= 0 && i - 2 * j < NTAPS)
                    {
#pragma unroll
                        for (int c = 0; c < 4; c++)
                            s[j][c] = mulAdd(s[j][c], taps.w[i - 2 * j], ev[c]);
                    }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                if constexpr (kHalf)
                {
                    if (4u * yg + j < tileH)
                        reinterpret_cast<Texel *>(dst + (size_t)(y0 + 4u * yg + j) * dstPitch)[x0 + x] = rangedTexel(s[j], lo);
                }
                else
                {
                    uint32_t out = plainByte<KIND>(s[j][3]) << 24;
                    if (RULE == kPlain)
                    {
#pragma unroll
                        for (int c = 0; c < 3; c++)
                            out |= plainByte<KIND>(s[j][c]) << (8 * c);
                    }
                    else if (RULE == kSrgb)
                    {
#pragma unroll
                        for (int c = 0; c < 3; c++)
                            out |= srgbEncode(tables, static_cast<uint32_t>(min(max((s[j][c] + (1 << 11)) >> 12, 0), 4 * 65535))) << (8 * c);
                    }
                    else
                    {
                        const int S[3] = {(s[j][0] + 128) >> 8, (s[j][1] + 128) >> 8, (s[j][2] + 128) >> 8};
                        if ((S[0] | S[1] | S[2]) == 0)
                        {
                            int p[3] = {0, 0, 0};
#pragma unroll
                            for (int k = 0; k < NTAPS; k++)
                            {
                                const short4 e = pbuf[(8u * yg + 2 * j + k) * kTileX + x];
                                p[0] += __mul24(taps.w[k], e.x);
                                p[1] += __mul24(taps.w[k], e.y);
                                p[2] += __mul24(taps.w[k], e.z);
                            }
#pragma unroll
                            for (int c = 0; c < 3; c++)
                                out |= plainByte<KIND>(p[c]) << (8 * c);
                        }
                        else
                        {
                            const float fx = static_cast<float>(S[0]), fy = static_cast<float>(S[1]), fz = static_cast<float>(S[2]);
                            const float f[3] = {fx, fy, fz};
                            const float len = sqrtf((fx * fx + fy * fy) + fz * fz); // (every operation rounds on its own: -ffp-contract=off)
#pragma unroll
                            for (int c = 0; c < 3; c++)
                                out |= normalByte<KIND>(f[c] / len) << (8 * c);
                        }
                    }
                    if (4u * yg + j < tileH)
                        reinterpret_cast<Texel *>(dst + (size_t)(y0 + 4u * yg + j) * dstPitch)[x0 + x] = out;
                }
            }
        }
        __syncthreads(); // the next tile's horizontal pass rewrites the entries
    }
}

// the taps of the kind from the Q14 table: the integers themselves, or (float)q * 2^-14 (exact)
template <int KIND, int RULE, int NTAPS>
hipError_t launchResample(const MipLayers &m, uint32_t wrap, const int16_t *taps, uint32_t range, hipStream_t stream)
{
    MipTaps<KIND> t;
    for (int k = 0; k < 12; k++)
    {
        if constexpr (KIND == kRGBA16F)
            t.w[k] = k < NTAPS ? static_cast<float>(taps[k]) * (1.0f / 16384.0f) : 0.0f;
        else
            t.w[k] = k < NTAPS ? taps[k] : 0;
    }
    const uint32_t dstW = m.srcW > 1u ? m.srcW >> 1 : 1u, dstH = m.srcH > 1u ? m.srcH >> 1 : 1u;
    // 16-byte reads: the first row and the pitch (and, for layers, the layer stride) on 16-byte boundaries -- the test of mipLaunchShape on
    // the source alone; the output is written a texel at a time
    uintptr_t bits = reinterpret_cast<uintptr_t>(m.src) | m.srcPitch;
    if (m.layers > 1u)
        bits |= m.srcLayer;
    const uint32_t wide = (bits & 15u) == 0 ? 1u : 0u;
    const uint32_t tilesY = (dstH + kTileY - 1u) / kTileY;
    const dim3 grid((dstW + kTileX - 1u) / kTileX, tilesY < 65535u ? tilesY : 65535u, m.layers);
    hipLaunchKernelGGL((cvttmi_mipresample_kernel<KIND, RULE, NTAPS>), grid, dim3(256), 0, stream, (const uint8_t *)m.src, m.srcPitch,
                       (uint8_t *)m.dst, m.dstPitch, m.srcW, m.srcH, dstW, dstH, m.srcLayer, m.dstLayer, wrap, wide, tilesY, t,
                       hdrRangeLow(range));
    return hipGetLastError();
}

// the pairs of withKindRule; anything else is hipErrorInvalidValue
hipError_t resampleByKind(const MipLayers &m, int kind, uint32_t rule, uint32_t wrap, uint32_t range, const int16_t *taps, uint32_t count,
                          hipStream_t stream)
{
    if (m.srcW == 0 || m.srcH == 0)
        return hipSuccess;
    if (!taps || count > 12u || !wrapOk(wrap) || !rangeFitsKind(kind, range))
        return hipErrorInvalidValue;
    return withKindRule(kind, rule, [&](auto k, auto r) {
        switch (count)
        {
        case 4: return launchResample<k(), r(), 4>(m, wrap, taps, range, stream);
        case 8: return launchResample<k(), r(), 8>(m, wrap, taps, range, stream);
        case 12: return launchResample<k(), r(), 12>(m, wrap, taps, range, stream);
        default: return hipErrorInvalidValue;
        }
    });
}
} // namespace

// One level of `layers` images (1 .. 65535, the layer in the grid's z) under a mip kernel: `rule` = CVTTMI_MIP_FILTER_BOX (the plain
// rule), _SRGB or _NORMAL, `wrap` = 0 or one CVTTMI_MIP_WRAP_* flag, `range` = one CVTTMI_MIP_HDR_* flag for RGBA16F and 0 otherwise,
// taps[0 .. count - 1] the kernel's Q14 table (count = 4, 8 or 12)
extern "C" hipError_t cvttmi_launch_resample(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch, size_t dstLayer,
                                             uint32_t srcW, uint32_t srcH, uint32_t layers, int kind, uint32_t rule, uint32_t wrap,
                                             uint32_t range, const int16_t *taps, uint32_t count, hipStream_t stream)
{
    if (!mipLayersOk(layers))
        return hipErrorInvalidValue;
    return resampleByKind(MipLayers{d_src, srcPitch, d_dst, dstPitch, srcW, srcH, srcLayer, dstLayer, layers}, kind, rule, wrap, range, taps, count,
                          stream);
}
