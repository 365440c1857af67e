// The mip filters beyond the box (include/cvtt_mi355x.h, "mip chains", CVTTMI_MIP_FILTER_*): one level per launch, the geometry,
// the launch shape and the wide / narrow split of mip_kernel.hip; RGBA8 and RGBA8_SNORM texels only.  Channel 3 (and whatever a
// rule sends back to the box rule) is box4x8 of the whole texel; channels 0..2 are replaced:
//   SRGB      S = T[a] + T[b] + T[c] + T[d], out = encode(S) = number of thresholds U[k] <= S (tools/gen_srgb_tables.py)
//   +ALPHA    the values (BOX) or T[values] (SRGB) weighted by the texels' alphas, exact unsigned divisions
//   NORMAL    integer sum of the four decoded vectors, one IEEE sqrt and three IEEE divisions, re-encoded
// The sRGB filters read their three tables from LDS (5.5 KB a workgroup, copied from constant memory by its 256 lanes): per
// output texel twelve 16-bit reads of T and, per channel, one byte of C[S >> 6] = encode(S with its low six bits cleared) and one
// threshold -- U's steps are above 64, so S passes at most one threshold more than its bucket's start.  No scratch.
#include "resample_common.h"
#include "cvtt_launchers.h"

namespace
{
// one output texel from its four input texels (channel i = bits 8 i .. 8 i + 7)
template <int KIND, int FILTER>
__device__ __forceinline__ uint32_t filterTexel(const SrgbTables &t, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t box = box4x8<KIND>(a, b, c, d);
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

// One output texel per lane: cvttmi_downsample_narrow_kernel with a filter (the layer in the grid's z there and here).
template <int KIND, int FILTER>
__global__ void __launch_bounds__(256) cvttmi_mipfilter_narrow_kernel(const uint8_t *__restrict__ src, size_t srcPitch,
                                                                       uint8_t *__restrict__ dst, size_t dstPitch, uint32_t srcW,
                                                                       uint32_t srcH, uint32_t dstW, uint32_t dstH, size_t srcLayer,
                                                                       size_t dstLayer)
{
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
        const uint32_t *r0 = reinterpret_cast<const uint32_t *>(src + (size_t)(2u * y) * srcPitch);
        const uint32_t *r1 = reinterpret_cast<const uint32_t *>(src + (size_t)min(2u * y + 1u, srcH - 1u) * srcPitch);
        reinterpret_cast<uint32_t *>(dst + (size_t)y * dstPitch)[x] = filterTexel<KIND, FILTER>(tables, r0[x0], r0[x1], r1[x0], r1[x1]);
    }
}

// Four output texels per lane, 16-byte accesses: cvttmi_downsample_wide_kernel with a filter (no clamp in x or y).
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
        const uint4 a = r0[0], b = r0[1], c = r1[0], d = r1[1]; // a = texels 0..3, b = texels 4..7
        uint4 o;
        o.x = filterTexel<KIND, FILTER>(tables, a.x, a.y, c.x, c.y);
        o.y = filterTexel<KIND, FILTER>(tables, a.z, a.w, c.z, c.w);
        o.z = filterTexel<KIND, FILTER>(tables, b.x, b.y, d.x, d.y);
        o.w = filterTexel<KIND, FILTER>(tables, b.z, b.w, d.z, d.w);
        reinterpret_cast<uint4 *>(dst + (size_t)y * dstPitch)[i] = o;
    }
}

template <int KIND, int FILTER>
hipError_t launchFiltered(const MipLayers &m, hipStream_t stream)
{
    const MipLaunch L = mipLaunchShape(m, 4u);
    if (L.wide)
        hipLaunchKernelGGL((cvttmi_mipfilter_wide_kernel<KIND, FILTER>), L.grid, L.block, 0, stream, (const uint8_t *)m.src,
                           m.srcPitch, (uint8_t *)m.dst, m.dstPitch, L.perRow, L.dstH, m.srcLayer, m.dstLayer);
    else
        hipLaunchKernelGGL((cvttmi_mipfilter_narrow_kernel<KIND, FILTER>), L.grid, L.block, 0, stream, (const uint8_t *)m.src,
                           m.srcPitch, (uint8_t *)m.dst, m.dstPitch, m.srcW, m.srcH, L.dstW, L.dstH, m.srcLayer, m.dstLayer);
    return hipGetLastError();
}

// the pairs of withKindFilter; anything else is hipErrorInvalidValue
hipError_t filteredByKind(const MipLayers &m, int kind, uint32_t filter, hipStream_t stream)
{
    if (m.srcW == 0 || m.srcH == 0)
        return hipSuccess;
    return withKindFilter(kind, filter, [&](auto k, auto f) { return launchFiltered<k(), f()>(m, stream); });
}
} // namespace

// cvttmi_launch_downsample under a filter other than the box (the shim sends CVTTMI_MIP_FILTER_BOX there)
extern "C" hipError_t cvttmi_launch_downsample_filtered(const void *d_src, size_t srcPitch, size_t srcLayer, void *d_dst, size_t dstPitch,
                                                        size_t dstLayer, uint32_t srcW, uint32_t srcH, uint32_t layers, int kind,
                                                        uint32_t filter, hipStream_t stream)
{
    if (!mipLayersOk(layers))
        return hipErrorInvalidValue;
    return filteredByKind(MipLayers{d_src, srcPitch, d_dst, dstPitch, srcW, srcH, srcLayer, dstLayer, layers}, kind, filter, stream);
}
