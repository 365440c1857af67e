// The 2x2 mip filters (include/cvtt_mi355x.h, "mip chains", CVTTMI_MIP_FILTER_*): one level per launch, level L+1 from level L.
//
// Output texel (x, y) is a function of input texels (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1), coordinates clamped to the
// input's last column / row (that only matters when a dimension is already 1; an odd dimension drops its last column / row).
// The box (the plain rule), for every pixel kind:
//   RGBA8        per channel (a + b + c + d + 2) >> 2 on unsigned bytes
//   RGBA8_SNORM  the same expression on the bytes read as int8, arithmetic shift: floor((sum + 2) / 4)
//   RGBA16F      half -> float, ((a + b) + (c + d)) * 0.25f in that order, float -> half round-to-nearest-even
// The other filters, RGBA8 and RGBA8_SNORM only: channel 3 (and whatever a rule sends back to the box rule) is box4x8 of the whole
// texel; channels 0..2 are replaced:
//   SRGB      S = T[a] + T[b] + T[c] + T[d], out = encode(S) = number of thresholds U[k] <= S (tools/gen_srgb_tables.py)
//   +ALPHA    the values (BOX) or T[values] (SRGB) weighted by the texels' alphas, exact unsigned divisions
//   NORMAL    integer sum of the four decoded vectors, one IEEE sqrt and three IEEE divisions, re-encoded
// The box is pure HBM traffic, 4 bytes in for 1 byte out.  Neighbouring lanes take neighbouring output texels.  The wide kernel
// gives a lane 16 bytes of output (four RGBA8 or two RGBA16F texels): two 16-byte loads from each of the two input rows, one
// 16-byte store.  It runs when both row starts, both pitches and the output width allow 16-byte accesses (mipLaunchShape);
// everything else takes the narrow kernel, one output texel per lane with texel-sized accesses.
// The sRGB filters read their three tables from LDS (5.5 KB a workgroup, copied from constant memory by its 256 lanes): per
// output texel twelve 16-bit reads of T and, per channel, one byte of C[S >> 6] = encode(S with its low six bits cleared) and one
// threshold -- U's steps are above 64, so S passes at most one threshold more than its bucket's start.  No other LDS, no scratch.
#include "resample_common.h"
#include "cvtt_launchers.h"

namespace
{
// RGBA16F: two halfs (one 32-bit word of a texel) at once, from the same word of the four input texels
__device__ __forceinline__ uint32_t box4x2h(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
        const int s = 16 * i;
        const float sum = (halfValue(a >> s) + halfValue(b >> s)) + (halfValue(c >> s) + halfValue(d >> s));
        // The compiler fuses the exact scaling and the conversion into one v_fma_mixlo_f16 (sum, 0.25, +0): one rounding, as
        // wanted, but -0 * 0.25 + +0 is +0.  The result has the sum's sign in every case, so that bit is taken from the sum.
        const uint32_t h = __builtin_bit_cast(uint16_t, static_cast<_Float16>(sum * 0.25f));
        out |= (h | ((__builtin_bit_cast(uint32_t, sum) >> 16) & 0x8000u)) << s;
    }
    return out;
}

// one output texel from its four input texels (channel i = bits 8 i .. 8 i + 7)
template <int KIND, int FILTER>
__device__ __forceinline__ uint32_t filterTexel(const SrgbTables &t, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t box = box4x8<KIND>(a, b, c, d);
    if (FILTER == kPlain)
        return box;
    if (FILTER == kNormal)
    {
        int s[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            s[ch] = ruleValue<KIND, kNormal>(a, ch, t.lin) + ruleValue<KIND, kNormal>(b, ch, t.lin) + ruleValue<KIND, kNormal>(c, ch, t.lin) +
                    ruleValue<KIND, kNormal>(d, ch, t.lin);
        const uint32_t Q = static_cast<uint32_t>(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]); // <= 3 * 1020^2 < 2^24: exact as a float
        if (Q == 0)
            return box;
        const float len = sqrtf(static_cast<float>(Q));
        uint32_t out = box & 0xff000000u;
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            out |= normalByte<KIND>(static_cast<float>(s[ch]) / len) << (8 * ch);
        return out;
    }
    const bool srgb = (FILTER & kSrgb) != 0, weighted = (FILTER & kAlphaWeighted) != 0;
    const uint32_t wa = a >> 24, wb = b >> 24, wc = c >> 24, wd = d >> 24;
    const uint32_t A = wa + wb + wc + wd, A1 = A ? A : 1u;
    uint32_t out = box & 0xff000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
    {
        uint32_t va = (a >> (8 * ch)) & 255u, vb = (b >> (8 * ch)) & 255u, vc = (c >> (8 * ch)) & 255u, vd = (d >> (8 * ch)) & 255u;
        if (srgb)
        {
            va = t.lin[va];
            vb = t.lin[vb];
            vc = t.lin[vc];
            vd = t.lin[vd];
        }
        uint32_t r;
        if (weighted)
        {
            const uint32_t N = va * wa + vb * wb + vc * wc + vd * wd; // srgb: 4 N <= 4 * 65535 * 1020 < 2^32
            if (srgb)
                r = srgbEncode(t, A ? (4u * N + (A >> 1)) / A1 : va + vb + vc + vd);
            else
                r = A ? (2u * N + A) / (2u * A1) : (box >> (8 * ch)) & 255u;
        }
        else
            r = srgbEncode(t, va + vb + vc + vd);
        out |= r << (8 * ch);
    }
    return out;
}

// One output texel per lane.  Texel = uint32_t or uint2 (RGBA16F, which has the box alone: a word of the output from the same
// word of the inputs).  Here and in the wide kernel workgroup z takes layer z of a texture array, `srcLayer` / `dstLayer` bytes
// further on (one image: z = 0).
template <int KIND, int FILTER>
__global__ void __launch_bounds__(256) cvttmi_mipfilter_narrow_kernel(const uint8_t *__restrict__ src, size_t srcPitch,
                                                                       uint8_t *__restrict__ dst, size_t dstPitch, uint32_t srcW,
                                                                       uint32_t srcH, uint32_t dstW, uint32_t dstH, size_t srcLayer,
                                                                       size_t dstLayer)
{
    typedef typename std::conditional<KIND == kRGBA16F, uint2, uint32_t>::type Texel;
    src += blockIdx.z * srcLayer;
    dst += blockIdx.z * dstLayer;
    __shared__ SrgbTables tables; // (no LDS is allocated where it is not read)
    if (FILTER & kSrgb)
    {
        loadSrgbTables(tables, blockDim.x * blockDim.y, threadIdx.y * blockDim.x + threadIdx.x);
        __syncthreads();
    }
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= dstW)
        return;
    const uint32_t x0 = 2u * x, x1 = min(2u * x + 1u, srcW - 1u); // 2x <= srcW - 1: dstW = max(1, srcW >> 1)
    for (uint32_t y = blockIdx.y * blockDim.y + threadIdx.y; y < dstH; y += gridDim.y * blockDim.y)
    {
        const Texel *r0 = reinterpret_cast<const Texel *>(src + (size_t)(2u * y) * srcPitch);
        const Texel *r1 = reinterpret_cast<const Texel *>(src + (size_t)min(2u * y + 1u, srcH - 1u) * srcPitch);
        Texel *row = reinterpret_cast<Texel *>(dst + (size_t)y * dstPitch);
        if constexpr (KIND == kRGBA16F)
        {
            const uint2 a = r0[x0], b = r0[x1], c = r1[x0], d = r1[x1];
            row[x] = make_uint2(box4x2h(a.x, b.x, c.x, d.x), box4x2h(a.y, b.y, c.y, d.y));
        }
        else
            row[x] = filterTexel<KIND, FILTER>(tables, r0[x0], r0[x1], r1[x0], r1[x1]);
    }
}

// 16 bytes of output per lane: chunk `i` of a row is output bytes [16 i, 16 i + 16) from input bytes [32 i, 32 i + 32) of
// rows 2y and 2y + 1.  chunks = dstW * texel bytes / 16, exact; the input rows hold at least 2 * dstW texels, so no clamp
// in x, and the launcher sends srcH == 1 to the narrow kernel, so none in y.
template <int KIND, int FILTER>
__global__ void __launch_bounds__(256) cvttmi_mipfilter_wide_kernel(const uint8_t *__restrict__ src, size_t srcPitch,
                                                                     uint8_t *__restrict__ dst, size_t dstPitch, uint32_t chunks,
                                                                     uint32_t dstH, size_t srcLayer, size_t dstLayer)
{
    src += blockIdx.z * srcLayer;
    dst += blockIdx.z * dstLayer;
    __shared__ SrgbTables tables;
    if (FILTER & kSrgb)
    {
        loadSrgbTables(tables, blockDim.x * blockDim.y, threadIdx.y * blockDim.x + threadIdx.x);
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= chunks)
        return;
    for (uint32_t y = blockIdx.y * blockDim.y + threadIdx.y; y < dstH; y += gridDim.y * blockDim.y)
    {
        const uint4 *r0 = reinterpret_cast<const uint4 *>(src + (size_t)(2u * y) * srcPitch) + 2u * i;
        const uint4 *r1 = reinterpret_cast<const uint4 *>(src + (size_t)(2u * y + 1u) * srcPitch) + 2u * i;
        const uint4 a = r0[0], b = r0[1], c = r1[0], d = r1[1];
        uint4 o;
        if constexpr (KIND == kRGBA16F)
        {
            // a = texels 0, 1 (two words each), b = texels 2, 3
            o.x = box4x2h(a.x, a.z, c.x, c.z);
            o.y = box4x2h(a.y, a.w, c.y, c.w);
            o.z = box4x2h(b.x, b.z, d.x, d.z);
            o.w = box4x2h(b.y, b.w, d.y, d.w);
        }
        else
        {
            // a = texels 0..3, b = texels 4..7
            o.x = filterTexel<KIND, FILTER>(tables, a.x, a.y, c.x, c.y);
            o.y = filterTexel<KIND, FILTER>(tables, a.z, a.w, c.z, c.w);
            o.z = filterTexel<KIND, FILTER>(tables, b.x, b.y, d.x, d.y);
            o.w = filterTexel<KIND, FILTER>(tables, b.z, b.w, d.z, d.w);
        }
        reinterpret_cast<uint4 *>(dst + (size_t)y * dstPitch)[i] = o;
    }
}

// `layers` (at most the z limit of a grid: the caller cuts longer arrays) images `srcLayer` / `dstLayer` bytes apart, one launch
// for all of them
template <int KIND, int FILTER>
hipError_t launchFiltered(const MipLayers &m, hipStream_t stream)
{
    const MipLaunch L = mipLaunchShape(m, KIND == kRGBA16F ? 8u : 4u);
    if (L.wide)
        hipLaunchKernelGGL((cvttmi_mipfilter_wide_kernel<KIND, FILTER>), L.grid, L.block, 0, stream, (const uint8_t *)m.src,
                           m.srcPitch, (uint8_t *)m.dst, m.dstPitch, L.perRow, L.dstH, m.srcLayer, m.dstLayer);
    else
        hipLaunchKernelGGL((cvttmi_mipfilter_narrow_kernel<KIND, FILTER>), L.grid, L.block, 0, stream, (const uint8_t *)m.src,
                           m.srcPitch, (uint8_t *)m.dst, m.dstPitch, m.srcW, m.srcH, L.dstW, L.dstH, m.srcLayer, m.dstLayer);
    return hipGetLastError();
}
} // namespace

// srcW x srcH texels at d_src (srcPitch bytes between rows) -> max(1, srcW >> 1) x max(1, srcH >> 1) texels at d_dst, of `layers`
// images (1 .. 65535) at once: layer z reads d_src + z * srcLayer and writes d_dst + z * dstLayer.
// kind: CVTTMI_PIXELS_RGBA8 / _RGBA16F / _RGBA8_SNORM; pointers and pitches are multiples of the texel size (the caller checks).
// filter: a pair of withKindFilter; anything else is hipErrorInvalidValue.
extern "C" hipError_t cvttmi_launch_downsample_filtered(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch,
                                                        size_t dstLayer, uint32_t srcW, uint32_t srcH, uint32_t layers, int kind,
                                                        uint32_t filter, hipStream_t stream)
{
    if (!mipLayersOk(layers))
        return hipErrorInvalidValue;
    if (srcW == 0 || srcH == 0)
        return hipSuccess;
    const MipLayers m = {d_src, srcPitch, d_dst, dstPitch, srcW, srcH, srcLayer, dstLayer, layers};
    return withKindFilter(kind, filter, [&](auto k, auto f) { return launchFiltered<k(), f()>(m, stream); });
}

// the box: the plain rule
extern "C" hipError_t cvttmi_launch_downsample(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch,
                                               size_t dstLayer, uint32_t srcW, uint32_t srcH, uint32_t layers, int kind, hipStream_t stream)
{
    return cvttmi_launch_downsample_filtered(d_src, srcPitch, srcLayer, d_dst, dstPitch, dstLayer, srcW, srcH, layers, kind, kPlain, stream);
}
