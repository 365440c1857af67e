// One mip level per launch: level L+1 = 2x2 box filter of level L (include/cvtt_mi355x.h, "mip chains").
//
// Output texel (x, y) averages input texels (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1), coordinates clamped to the
// input's last column / row (that only matters when a dimension is already 1; an odd dimension drops its last column / row).
//   RGBA8        per channel (a + b + c + d + 2) >> 2 on unsigned bytes
//   RGBA8_SNORM  the same expression on the bytes read as int8, arithmetic shift: floor((sum + 2) / 4)
//   RGBA16F      half -> float, ((a + b) + (c + d)) * 0.25f in that order, float -> half round-to-nearest-even
// Pure HBM traffic, 4 bytes in for 1 byte out.  Neighbouring lanes take neighbouring output texels.  The wide kernel gives a
// lane 16 bytes of output (four RGBA8 or two RGBA16F texels): two 16-byte loads from each of the two input rows, one 16-byte
// store.  It runs when both row starts, both pitches and the output width allow 16-byte accesses; everything else takes the
// narrow kernel, one output texel per lane with texel-sized accesses.  No LDS, no scratch.
#include "mip_common.h"
#include "cvtt_launchers.h"

namespace
{
__device__ __forceinline__ float halfToFloat(uint32_t bits)
{
    return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(bits)));
}

// two halfs (one 32-bit word of a texel) at once
__device__ __forceinline__ uint32_t box4x2h(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
        const int s = 16 * i;
        const float sum = (halfToFloat(a >> s) + halfToFloat(b >> s)) + (halfToFloat(c >> s) + halfToFloat(d >> s));
        // The compiler fuses the exact scaling and the conversion into one v_fma_mixlo_f16 (sum, 0.25, +0): one rounding, as
        // wanted, but -0 * 0.25 + +0 is +0.  The result has the sum's sign in every case, so that bit is taken from the sum.
        const uint32_t h = __builtin_bit_cast(uint16_t, static_cast<_Float16>(sum * 0.25f));
        out |= (h | ((__builtin_bit_cast(uint32_t, sum) >> 16) & 0x8000u)) << s;
    }
    return out;
}

// one 32-bit word of an output texel from the same word of its four input texels
template <int KIND>
__device__ __forceinline__ uint32_t boxWord(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    return KIND == kRGBA16F ? box4x2h(a, b, c, d) : box4x8<KIND>(a, b, c, d);
}

// One output texel per lane.  Texel = uint32_t (RGBA8) or uint2 (RGBA16F).
// Here and in the wide kernel workgroup z takes layer z of a texture array, `srcLayer` / `dstLayer` bytes further on (one image: z = 0).
template <int KIND>
__global__ void __launch_bounds__(256) cvttmi_downsample_narrow_kernel(const uint8_t *__restrict__ src, size_t srcPitch,
                                                                        uint8_t *__restrict__ dst, size_t dstPitch, uint32_t srcW,
                                                                        uint32_t srcH, uint32_t dstW, uint32_t dstH, size_t srcLayer,
                                                                        size_t dstLayer)
{
    src += blockIdx.z * srcLayer;
    dst += blockIdx.z * dstLayer;
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= dstW)
        return;
    const uint32_t x0 = 2u * x, x1 = min(2u * x + 1u, srcW - 1u); // 2x <= srcW - 1: dstW = max(1, srcW >> 1)
    for (uint32_t y = blockIdx.y * blockDim.y + threadIdx.y; y < dstH; y += gridDim.y * blockDim.y)
    {
        const uint8_t *r0 = src + (size_t)(2u * y) * srcPitch;
        const uint8_t *r1 = src + (size_t)min(2u * y + 1u, srcH - 1u) * srcPitch;
        if (KIND == kRGBA16F)
        {
            const uint2 a = reinterpret_cast<const uint2 *>(r0)[x0], b = reinterpret_cast<const uint2 *>(r0)[x1];
            const uint2 c = reinterpret_cast<const uint2 *>(r1)[x0], d = reinterpret_cast<const uint2 *>(r1)[x1];
            reinterpret_cast<uint2 *>(dst + (size_t)y * dstPitch)[x] =
                make_uint2(boxWord<KIND>(a.x, b.x, c.x, d.x), boxWord<KIND>(a.y, b.y, c.y, d.y));
        }
        else
        {
            const uint32_t a = reinterpret_cast<const uint32_t *>(r0)[x0], b = reinterpret_cast<const uint32_t *>(r0)[x1];
            const uint32_t c = reinterpret_cast<const uint32_t *>(r1)[x0], d = reinterpret_cast<const uint32_t *>(r1)[x1];
            reinterpret_cast<uint32_t *>(dst + (size_t)y * dstPitch)[x] = boxWord<KIND>(a, b, c, d);
        }
    }
}

// 16 bytes of output per lane: chunk `i` of a row is output bytes [16 i, 16 i + 16) from input bytes [32 i, 32 i + 32) of
// rows 2y and 2y + 1.  chunks = dstW * texel bytes / 16, exact; the input rows hold at least 2 * dstW texels, so no clamp
// in x, and the launcher sends srcH == 1 to the narrow kernel, so none in y.
template <int KIND>
__global__ void __launch_bounds__(256) cvttmi_downsample_wide_kernel(const uint8_t *__restrict__ src, size_t srcPitch,
                                                                      uint8_t *__restrict__ dst, size_t dstPitch, uint32_t chunks,
                                                                      uint32_t dstH, size_t srcLayer, size_t dstLayer)
{
    src += blockIdx.z * srcLayer;
    dst += blockIdx.z * dstLayer;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= chunks)
        return;
    for (uint32_t y = blockIdx.y * blockDim.y + threadIdx.y; y < dstH; y += gridDim.y * blockDim.y)
    {
        const uint4 *r0 = reinterpret_cast<const uint4 *>(src + (size_t)(2u * y) * srcPitch) + 2u * i;
        const uint4 *r1 = reinterpret_cast<const uint4 *>(src + (size_t)(2u * y + 1u) * srcPitch) + 2u * i;
        const uint4 a = r0[0], b = r0[1], c = r1[0], d = r1[1];
        uint4 o;
        if (KIND == kRGBA16F)
        {
            // a = texels 0, 1 (two words each), b = texels 2, 3
            o.x = boxWord<KIND>(a.x, a.z, c.x, c.z);
            o.y = boxWord<KIND>(a.y, a.w, c.y, c.w);
            o.z = boxWord<KIND>(b.x, b.z, d.x, d.z);
            o.w = boxWord<KIND>(b.y, b.w, d.y, d.w);
        }
        else
        {
            // a = texels 0..3, b = texels 4..7
            o.x = boxWord<KIND>(a.x, a.y, c.x, c.y);
            o.y = boxWord<KIND>(a.z, a.w, c.z, c.w);
            o.z = boxWord<KIND>(b.x, b.y, d.x, d.y);
            o.w = boxWord<KIND>(b.z, b.w, d.z, d.w);
        }
        reinterpret_cast<uint4 *>(dst + (size_t)y * dstPitch)[i] = o;
    }
}

// `layers` (at most the z limit of a grid: the caller cuts longer arrays) images `srcLayer` / `dstLayer` bytes apart, one launch
// for all of them
template <int KIND>
hipError_t launchDownsample(const MipLayers &m, hipStream_t stream)
{
    const MipLaunch L = mipLaunchShape(m, KIND == kRGBA16F ? 8u : 4u);
    if (L.wide)
        hipLaunchKernelGGL((cvttmi_downsample_wide_kernel<KIND>), L.grid, L.block, 0, stream, (const uint8_t *)m.src, m.srcPitch,
                           (uint8_t *)m.dst, m.dstPitch, L.perRow, L.dstH, m.srcLayer, m.dstLayer);
    else
        hipLaunchKernelGGL((cvttmi_downsample_narrow_kernel<KIND>), L.grid, L.block, 0, stream, (const uint8_t *)m.src, m.srcPitch,
                           (uint8_t *)m.dst, m.dstPitch, m.srcW, m.srcH, L.dstW, L.dstH, m.srcLayer, m.dstLayer);
    return hipGetLastError();
}

hipError_t downsampleByKind(const MipLayers &m, int kind, hipStream_t stream)
{
    if (m.srcW == 0 || m.srcH == 0)
        return hipSuccess;
    switch (kind)
    {
    case kRGBA8: return launchDownsample<kRGBA8>(m, stream);
    case kRGBA16F: return launchDownsample<kRGBA16F>(m, stream);
    case kRGBA8Snorm: return launchDownsample<kRGBA8Snorm>(m, stream);
    default: return hipErrorInvalidValue;
    }
}
} // namespace

// srcW x srcH texels at d_src (srcPitch bytes between rows) -> max(1, srcW >> 1) x max(1, srcH >> 1) texels at d_dst, of `layers`
// images (1 .. 65535) at once: layer z reads d_src + z * srcLayer and writes d_dst + z * dstLayer.
// kind: CVTTMI_PIXELS_RGBA8 / _RGBA16F / _RGBA8_SNORM; pointers and pitches are multiples of the texel size (the caller checks).
extern "C" hipError_t cvttmi_launch_downsample(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch,
                                               size_t dstLayer, uint32_t srcW, uint32_t srcH, uint32_t layers, int kind, hipStream_t stream)
{
    if (!mipLayersOk(layers))
        return hipErrorInvalidValue;
    return downsampleByKind(MipLayers{d_src, srcPitch, d_dst, dstPitch, srcW, srcH, srcLayer, dstLayer, layers}, kind, stream);
}
