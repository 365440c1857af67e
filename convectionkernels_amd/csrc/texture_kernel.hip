// Texture arrays and cube maps (include/cvtt_mi355x.h, "texture arrays and cube maps"): the data movement around ONE search
// over every level of every layer.  Two kernels, one launch each for the whole texture, whatever its layers and levels:
//
//   chain tile     every level of every layer -> one PixelBlock buffer, groups of eight horizontally adjacent 4x4 blocks with
//                  the edge clamp of cvttmi_tile_kernel (tile_kernel.hip).  A lane moves one four-texel row of one block
//                  (16 B of RGBA8, 32 B of RGBA16F).  Lanes are numbered layer, level, texel row, block: the tilesPerRow
//                  lanes that share a texel row of a level are neighbours and read one contiguous run of that image row, as
//                  in the single-image kernel -- a wave of a narrow level takes several texel rows, a run each.
//   chain compact  the padded packed blocks of every (layer, level) -> their place in the output, layer-major (DDS) or
//                  level-major (KTX): cvttmi_texture_subresource's two formulas.  A lane moves one block, 8 or 16 bytes.
//
// A lane finds its layer by one division and its level by a scan of the level table, which travels by value as a kernel
// argument (CvttTextureLevels, cvtt_device.h) like the decoder's (cvttmi_decode_mips_kernel).  Pure HBM copies: no LDS, no
// atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cvtt_device.h"
#include "cvtt_launchers.h"

namespace
{
const uint32_t kChainWG = 256;

template <int BYTES_PER_PIXEL>
__global__ __launch_bounds__(256) void cvttmi_tile_chain_kernel(const CvttTextureLevels T, uint8_t *__restrict__ tiles)
{
    const uint64_t lanesPerLayer = 4ull * T.tilesPerLayer;
    const uint64_t t = (uint64_t)blockIdx.x * kChainWG + threadIdx.x;
    const uint32_t layer = (uint32_t)(t / lanesPerLayer);
    if (layer >= T.layers)
        return;
    const uint64_t r = t - (uint64_t)layer * lanesPerLayer; // lane inside the layer: 4 lanes a tile
    uint32_t l = 0;
    for (uint32_t i = 1; i < T.count; i++)
        l = r >= 4ull * T.level[i].firstTile ? i : l;
    const CvttTextureLevel &L = T.level[l];
    const uint64_t q = r - 4ull * L.firstTile;
    const uint32_t row = (uint32_t)(q / L.tilesPerRow); // texel row of the level, padded to whole blocks: 4 by + subY
    const uint32_t bx = (uint32_t)(q - (uint64_t)row * L.tilesPerRow);
    const uint32_t by = row >> 2, subY = row & 3u;
    const uint32_t y = min(row, L.height - 1u);
    const uint8_t *src = L.image + (size_t)layer * L.layerStride + (size_t)y * L.pitch;
    uint8_t *dst = tiles + ((size_t)layer * T.tilesPerLayer + L.firstTile + (size_t)by * L.tilesPerRow + bx) * (16u * BYTES_PER_PIXEL) +
                   subY * (4u * BYTES_PER_PIXEL);
    typedef typename std::conditional<BYTES_PER_PIXEL == 4, uint32_t, uint2>::type Pixel;
    const Pixel *in = reinterpret_cast<const Pixel *>(src);
    Pixel px[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        px[i] = in[min(bx * 4u + (uint32_t)i, L.width - 1u)];
    Pixel *out = reinterpret_cast<Pixel *>(dst);
#pragma unroll
    for (int i = 0; i < 4; i++)
        out[i] = px[i];
}

// Unit = one packed block: uint2 (8 bytes) or uint4 (16 bytes)
template <class Unit>
__global__ __launch_bounds__(256) void cvttmi_compact_chain_kernel(const CvttTextureLevels T, const Unit *__restrict__ packed,
                                                                   Unit *__restrict__ out)
{
    const uint64_t u = (uint64_t)blockIdx.x * kChainWG + threadIdx.x; // block of the layer-major output
    const uint32_t layer = (uint32_t)(u / T.blocksPerLayer);
    if (layer >= T.layers)
        return;
    const uint32_t r = (uint32_t)(u - (uint64_t)layer * T.blocksPerLayer);
    uint32_t l = 0;
    for (uint32_t i = 1; i < T.count; i++)
        l = r >= T.level[i].firstBlock ? i : l;
    const CvttTextureLevel &L = T.level[l];
    const uint32_t q = r - L.firstBlock, by = q / L.blocksPerRow, bx = q - by * L.blocksPerRow;
    const size_t src = (size_t)layer * T.tilesPerLayer + L.firstTile + (size_t)by * L.tilesPerRow + bx;
    // cvttmi_texture_subresource: layer * E + firstBlock, or layers * firstBlock + layer * blockCount
    const size_t dst = T.levelMajor ? (size_t)T.layers * L.firstBlock + (size_t)layer * L.blockCount + q : (size_t)u;
    out[dst] = packed[src];
}

uint32_t chainGrid(uint64_t lanes) { return (uint32_t)((lanes + kChainWG - 1u) / kChainWG); }
} // namespace

// levels: the table of the texture; d_tiles: layers x tilesPerLayer PixelBlocks of 16 x bytesPerPixel bytes
extern "C" hipError_t cvttmi_launch_tile_chain(const CvttTextureLevels *levels, void *d_tiles, uint32_t bytesPerPixel, hipStream_t stream)
{
    const uint64_t lanes = 4ull * levels->tilesPerLayer * levels->layers; // below 2^34: 2^26 workgroups at the most
    if (lanes == 0)
        return hipSuccess;
    if (bytesPerPixel == 4)
        hipLaunchKernelGGL(cvttmi_tile_chain_kernel<4>, dim3(chainGrid(lanes)), dim3(kChainWG), 0, stream, *levels, (uint8_t *)d_tiles);
    else
        hipLaunchKernelGGL(cvttmi_tile_chain_kernel<8>, dim3(chainGrid(lanes)), dim3(kChainWG), 0, stream, *levels, (uint8_t *)d_tiles);
    return hipGetLastError();
}

// d_packed: layers x tilesPerLayer packed blocks as the search leaves them; d_out: layers x blocksPerLayer blocks in
// levels->levelMajor's order.  bytesPerBlock: 8 or 16.
extern "C" hipError_t cvttmi_launch_compact_chain(const CvttTextureLevels *levels, const void *d_packed, void *d_out, uint32_t bytesPerBlock,
                                                  hipStream_t stream)
{
    const uint64_t blocks = (uint64_t)levels->blocksPerLayer * levels->layers;
    if (blocks == 0)
        return hipSuccess;
    if (bytesPerBlock == 8)
        hipLaunchKernelGGL(cvttmi_compact_chain_kernel<uint2>, dim3(chainGrid(blocks)), dim3(kChainWG), 0, stream, *levels,
                           (const uint2 *)d_packed, (uint2 *)d_out);
    else
        hipLaunchKernelGGL(cvttmi_compact_chain_kernel<uint4>, dim3(chainGrid(blocks)), dim3(kChainWG), 0, stream, *levels,
                           (const uint4 *)d_packed, (uint4 *)d_out);
    return hipGetLastError();
}
