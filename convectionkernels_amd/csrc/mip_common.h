// What the mip and resize kernels share before any rule (resample_common.h includes it, and every kernel file includes that): the
// pixel kinds, the box rule on four bytes at once, and the shape of a level's launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace
{
enum
{
    kRGBA8 = 0,
    kRGBA16F = 1,
    kRGBA8Snorm = 2
};

// four bytes at once: even and odd bytes are summed in 16-bit fields (4 * 255 + 2 fits).  int8 bytes become offset binary
// (v + 128) first: the four offsets add 512, a multiple of 4, so the unsigned rule gives floor((sum + 2) / 4) + 128.
template <int KIND>
__device__ __forceinline__ uint32_t box4x8(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t bias = KIND == kRGBA8Snorm ? 0x80808080u : 0u;
    a ^= bias;
    b ^= bias;
    c ^= bias;
    d ^= bias;
    const uint32_t m = 0x00ff00ffu;
    const uint32_t even = (a & m) + (b & m) + (c & m) + (d & m) + 0x00020002u;
    const uint32_t odd = ((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m) + 0x00020002u;
    return (((even >> 2) & m) | (((odd >> 2) & m) << 8)) ^ bias;
}

// What one level's launch reads and writes: the same level of `layers` images (1 .. kMipMaxLayers; one image is a texture array of
// one layer), srcLayer / dstLayer bytes apart, layer z in workgroups z of the grid.
struct MipLayers
{
    const void *src;
    size_t srcPitch;
    void *dst;
    size_t dstPitch;
    uint32_t srcW, srcH;
    size_t srcLayer, dstLayer;
    uint32_t layers;
};
const uint32_t kMipMaxLayers = 65535; // the z limit of a grid
inline bool mipLayersOk(uint32_t layers)
{
    return layers != 0 && layers <= kMipMaxLayers;
}

// One level's launch.  The wide kernel (16 bytes of output per lane) runs when both row starts, both pitches and the output
// width allow 16-byte accesses and no coordinate needs a clamp -- for every layer: the two layer strides enter the same test
// (with the first layer's rows and both strides on 16-byte boundaries every layer's rows are); everything else takes the
// narrow one, a texel per lane.
struct MipLaunch
{
    bool wide;
    uint32_t dstW, dstH, perRow; // perRow: lanes of one output row
    dim3 grid, block;
};

inline MipLaunch mipLaunchShape(const MipLayers &m, uint32_t texel)
{
    const uint32_t srcW = m.srcW, srcH = m.srcH;
    MipLaunch L;
    L.dstW = srcW > 1u ? srcW >> 1 : 1u;
    L.dstH = srcH > 1u ? srcH >> 1 : 1u;
    uintptr_t bits = reinterpret_cast<uintptr_t>(m.src) | reinterpret_cast<uintptr_t>(m.dst) | m.srcPitch | m.dstPitch |
                     ((uintptr_t)L.dstW * texel);
    if (m.layers > 1u)
        bits |= m.srcLayer | m.dstLayer;
    L.wide = (bits & 15u) == 0 && srcW >= 2u && srcH >= 2u;
    L.perRow = L.wide ? L.dstW / (16u / texel) : L.dstW;
    // a workgroup of 256 lanes, as wide as the row needs (a power of two) and as many rows high as that leaves; at most 1024
    // workgroups down the image (enough to fill the device at any width), the kernels' row loop takes the rows beyond
    uint32_t bx = 1;
    while (bx < L.perRow && bx < 256u)
        bx *= 2u;
    const uint32_t by = 256u / bx;
    const uint32_t gy = (L.dstH + by - 1u) / by;
    L.block = dim3(bx, by);
    L.grid = dim3((L.perRow + bx - 1u) / bx, gy < 1024u ? gy : 1024u, m.layers);
    return L;
}
} // namespace
