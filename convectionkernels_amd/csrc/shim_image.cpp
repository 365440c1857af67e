// Images on the device (cvtt_mi355x.h: tiling, "mip chains", "texture arrays and cube maps", "resize"): tile and compact, the mip
// layout and taps, the one level loop, and the build-mips, texture and resize entries.
#include "shim_internal.h"

#include <math.h>
#include <vector>

#include "srgb_tables.h"
#include "mip_kernel_tables.h"

using namespace cvtt_shim;

namespace
{
    // bytes of one texel of a mip chain's pixel kind (CVTTMI_PIXELS_*); 0 = unknown kind
    size_t mipTexelBytes(int pixelFormat)
    {
        return (pixelFormat == CVTTMI_PIXELS_RGBA8 || pixelFormat == CVTTMI_PIXELS_RGBA8_SNORM) ? 4u : pixelFormat == CVTTMI_PIXELS_RGBA16F ? 8u : 0u;
    }
    // the filters a pixel kind takes (cvtt_mi355x.h, CVTTMI_MIP_FILTER_*, CVTTMI_MIP_KERNEL_*, CVTTMI_MIP_WRAP_*)
    // A filter word's four fields: `rule` is everything outside the other three (BOX, SRGB or NORMAL, ALPHA_WEIGHTED with them, and
    // any bit that means nothing), `code` the kernel (0 = none), `wrap` the wrap flags and `range` the CVTTMI_MIP_HDR_* flags as they
    // stand in the word.
    struct FilterWord
    {
        uint32_t rule, code, wrap, range;
    };
    FilterWord splitFilter(uint32_t filter)
    {
        const uint32_t kernel = 0xf0u, wrap = CVTTMI_MIP_WRAP_REPEAT | CVTTMI_MIP_WRAP_MIRROR;
        const uint32_t range = CVTTMI_MIP_HDR_NONNEGATIVE | CVTTMI_MIP_HDR_SIGNED;
        return FilterWord{filter & ~(kernel | wrap | range), (filter & kernel) >> 4, filter & wrap, filter & range};
    }
    bool oneWrapAtMost(uint32_t wrap)
    {
        return wrap != (CVTTMI_MIP_WRAP_REPEAT | CVTTMI_MIP_WRAP_MIRROR);
    }
    // does the pixel kind take the rule and the range under a kernel (in a mip chain or a resize)?  No ALPHA_WEIGHTED there; RGBA16F
    // takes the plain rule with exactly one range flag, and a range flag goes with nothing else.  The (kind, rule) pairs that exist
    // are the kernels' list (resample_common.h, withKindRule): a pair has an entry size, anything else 0.
    bool kernelRuleFits(int pixelFormat, uint32_t rule, uint32_t range)
    {
        const bool oneFlag = range == CVTTMI_MIP_HDR_NONNEGATIVE || range == CVTTMI_MIP_HDR_SIGNED;
        return cvttmi_resize_entry_bytes(pixelFormat, rule) != 0 && (pixelFormat == CVTTMI_PIXELS_RGBA16F ? oneFlag : range == 0);
    }
    // the tap table of a mip kernel and its length; NULL for kernel 0 and unknown kernels
    const int16_t *mipKernelTaps(uint32_t code, uint32_t *count)
    {
        if (code == 0 || code > CVTT_MIP_KERNELS)
            return NULL;
        *count = k_mipKernelTapCount[code - 1];
        return k_mipKernelTaps[code - 1];
    }
    bool mipFilterFits(int pixelFormat, uint32_t filter) // pixelFormat: one mipTexelBytes knows
    {
        const FilterWord f = splitFilter(filter);
        uint32_t count;
        if (f.code || f.wrap) // a kernel; a wrap flag alone is nothing
            return mipKernelTaps(f.code, &count) && oneWrapAtMost(f.wrap) && kernelRuleFits(pixelFormat, f.rule, f.range);
        if (f.range) // a range flag without a kernel: the 2x2 rules have no range
            return false;
        if (f.rule == CVTTMI_MIP_FILTER_BOX)
            return true;
        if (f.rule == CVTTMI_MIP_FILTER_NORMAL)
            return pixelFormat != CVTTMI_PIXELS_RGBA16F;
        return pixelFormat == CVTTMI_PIXELS_RGBA8 && (f.rule == CVTTMI_MIP_FILTER_SRGB || f.rule == (CVTTMI_MIP_FILTER_BOX | CVTTMI_MIP_FILTER_ALPHA_WEIGHTED) ||
                                                      f.rule == (CVTTMI_MIP_FILTER_SRGB | CVTTMI_MIP_FILTER_ALPHA_WEIGHTED));
    }
    const char *const kMipFilterText =
        "mip filter: RGBA8 takes BOX, SRGB, either with ALPHA_WEIGHTED, and NORMAL; RGBA8_SNORM BOX and NORMAL; RGBA16F BOX; a "
        "CVTTMI_MIP_KERNEL_* goes with BOX, SRGB or NORMAL of RGBA8 / RGBA8_SNORM and with BOX of RGBA16F, which then needs exactly one "
        "CVTTMI_MIP_HDR_* flag (a flag goes with nothing else); one CVTTMI_MIP_WRAP_* flag only with a kernel";
}

extern "C"
{
    size_t cvttmi_tiled_block_count(uint32_t width, uint32_t height)
    {
        const size_t perRow = (((size_t)width + 3) / 4 + 7) / 8 * 8;
        return perRow * (((size_t)height + 3) / 4);
    }

    int cvttmi_tile_image_device(cvttmi_context *ctx, void *d_blocks, const void *d_image, uint32_t width, uint32_t height,
                                 size_t rowPitchBytes, int pixelFormat, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        const uint32_t bpp = (pixelFormat == CVTTMI_PIXELS_RGBA8) ? 4u : (pixelFormat == CVTTMI_PIXELS_RGBA16F) ? 8u : 0u;
        if (!d_blocks || !d_image || bpp == 0 || width == 0 || height == 0 || rowPitchBytes < (size_t)width * bpp ||
            (rowPitchBytes % bpp) != 0)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (!alignedTo(d_blocks, 16u * bpp) || !alignedTo(d_image, bpp))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        return withDevice(ctx, [&] {
            const hipError_t e = cvttmi_launch_tile(d_image, d_blocks, width, height, rowPitchBytes, bpp, static_cast<hipStream_t>(hipStream));
            return e == hipSuccess ? CVTTMI_OK : fail(ctx, CVTTMI_E_HIP, "tile kernel launch", e);
        });
    }

    int cvttmi_compact_rows_device(cvttmi_context *ctx, void *d_out, const void *d_packed, uint32_t width, uint32_t height,
                                   uint32_t bytesPerBlock, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        if (!d_out || !d_packed || width == 0 || height == 0 || (bytesPerBlock != 8 && bytesPerBlock != 16))
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (!alignedTo(d_out, bytesPerBlock) || !alignedTo(d_packed, bytesPerBlock))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        return withDevice(ctx, [&] {
            const hipError_t e = cvttmi_launch_compact_rows(d_packed, d_out, width, height, bytesPerBlock, static_cast<hipStream_t>(hipStream));
            return e == hipSuccess ? CVTTMI_OK : fail(ctx, CVTTMI_E_HIP, "compact kernel launch", e);
        });
    }

    // ---- mip chains (cvtt_mi355x.h, "mip chains"): the level sizes and the three layouts, and the level images ----
    uint32_t cvttmi_mip_level_count(uint32_t width, uint32_t height)
    {
        if (width == 0 || height == 0)
            return 0;
        uint32_t levels = 1;
        for (uint32_t m = width > height ? width : height; m > 1; m >>= 1)
            levels++;
        return levels;
    }

    int cvttmi_mip_layout(uint32_t width, uint32_t height, int pixelFormat, uint32_t bytesPerBlock, uint32_t levels, cvttmi_mip_level *out)
    {
        const size_t texel = mipTexelBytes(pixelFormat);
        if (!out || texel == 0 || (bytesPerBlock != 8 && bytesPerBlock != 16) || levels == 0 || levels > cvttmi_mip_level_count(width, height))
            return CVTTMI_E_INVALID;
        // computed into a copy: nothing is written when a size does not fit a size_t
        cvttmi_mip_level table[kMaxMipLevels + 1];
        size_t bytes = 0, tiles = 0, blocks = 0;
        uint32_t w = width, h = height;
        for (uint32_t l = 0; l < levels; l++)
        {
            cvttmi_mip_level &L = table[l];
            memset(&L, 0, sizeof(L));
            L.width = w;
            L.height = h;
            if (l > 0)
            {
                size_t size;
                L.rowPitchBytes = (size_t)w * texel;
                if (__builtin_mul_overflow(L.rowPitchBytes, (size_t)h, &size) || __builtin_add_overflow(bytes, size, &size) ||
                    size > SIZE_MAX - 255)
                    return CVTTMI_E_INVALID;
                L.byteOffset = bytes;
                bytes = (size + 255) / 256 * 256; // where the next level starts
                if (l + 1 == levels)
                    bytes = size; // ... and the last one ends the pyramid
            }
            L.firstTile = tiles;
            L.tileCount = cvttmi_tiled_block_count(w, h);
            L.firstBlock = blocks;
            L.blockCount = (((size_t)w + 3) / 4) * (((size_t)h + 3) / 4);
            L.packedByteOffset = blocks * bytesPerBlock;
            tiles += L.tileCount;
            blocks += L.blockCount;
            w = w > 1 ? w >> 1 : 1;
            h = h > 1 ? h >> 1 : 1;
        }
        cvttmi_mip_level &T = table[levels];
        memset(&T, 0, sizeof(T));
        T.byteOffset = bytes;
        T.firstTile = tiles;
        T.firstBlock = blocks;
        T.packedByteOffset = blocks * bytesPerBlock;
        memcpy(out, table, sizeof(cvttmi_mip_level) * (levels + 1));
        return CVTTMI_OK;
    }

    int cvttmi_srgb_tables(uint16_t toLinear[256], uint32_t thresholds[255])
    {
        if (!toLinear || !thresholds)
            return CVTTMI_E_INVALID;
        static_assert(sizeof(k_srgbToLinear) == 256 * sizeof(uint16_t) && sizeof(k_srgbThresholds) == 255 * sizeof(uint32_t), "srgb_tables.h");
        memcpy(toLinear, k_srgbToLinear, sizeof(k_srgbToLinear));
        memcpy(thresholds, k_srgbThresholds, sizeof(k_srgbThresholds));
        return CVTTMI_OK;
    }

    int cvttmi_mip_kernel_taps(uint32_t filter, int16_t taps[12], uint32_t *count)
    {
        uint32_t n = 0;
        const int16_t *table = mipKernelTaps(splitFilter(filter).code, &n);
        if (!table || !taps || !count)
            return CVTTMI_E_INVALID;
        static_assert(sizeof(k_mipKernelTaps[0]) == 12 * sizeof(int16_t), "mip_kernel_tables.h");
        memcpy(taps, table, sizeof(k_mipKernelTaps[0]));
        *count = n;
        return CVTTMI_OK;
    }

    // Levels 1 .. of every layer into d_pyramids, a layer's pyramid pyramidLayerBytes after the one before: one launch per level for
    // all layers (per 65535 of them).  The one level loop of the library: a single image is one layer.  Arguments checked.
    static int queueMips(cvttmi_context *ctx, uint8_t *d_pyramids, size_t pyramidLayerBytes, const cvttmi_mip_level *table,
                         const uint8_t *d_images, size_t rowPitchBytes, size_t layerPitchBytes, int pixelFormat, uint32_t levels, uint32_t layers,
                         uint32_t filter, hipStream_t stream)
    {
        const uint32_t kGridLayers = 65535; // the z limit of a grid
        // a kernel's table with the rule and the wrap, else a 2x2 filter, the box among them (mipFilterFits has passed the word)
        const FilterWord f = splitFilter(filter);
        uint32_t tapCount = 0;
        const int16_t *taps = mipKernelTaps(f.code, &tapCount);
        for (uint32_t first = 0; first < layers; first += kGridLayers)
        {
            const uint32_t n = layers - first < kGridLayers ? layers - first : kGridLayers;
            const uint8_t *src = d_images + (size_t)first * layerPitchBytes;
            size_t srcPitch = rowPitchBytes, srcLayer = layerPitchBytes;
            for (uint32_t l = 1; l < levels; l++)
            {
                uint8_t *dst = d_pyramids + (size_t)first * pyramidLayerBytes + table[l].byteOffset;
                const hipError_t e =
                    taps ? cvttmi_launch_resample(src, srcPitch, srcLayer, dst, table[l].rowPitchBytes, pyramidLayerBytes, table[l - 1].width,
                                                  table[l - 1].height, n, pixelFormat, f.rule, f.wrap, f.range, taps, tapCount, stream)
                         : cvttmi_launch_downsample_filtered(src, srcPitch, srcLayer, dst, table[l].rowPitchBytes, pyramidLayerBytes,
                                                             table[l - 1].width, table[l - 1].height, n, pixelFormat, f.rule, stream);
                if (e != hipSuccess)
                    return fail(ctx, CVTTMI_E_HIP, "downsample kernel launch", e);
                src = dst;
                srcPitch = table[l].rowPitchBytes;
                srcLayer = pyramidLayerBytes;
            }
        }
        return CVTTMI_OK;
    }

    int cvttmi_build_mips_device(cvttmi_context *ctx, void *d_pyramid, size_t pyramidBytes, const void *d_image, uint32_t width,
                                 uint32_t height, size_t rowPitchBytes, int pixelFormat, uint32_t levels, void *hipStream)
    {
        return cvttmi_build_mips_filtered_device(ctx, d_pyramid, pyramidBytes, d_image, width, height, rowPitchBytes, pixelFormat, levels,
                                                 CVTTMI_MIP_FILTER_BOX, hipStream);
    }

    int cvttmi_build_mips_filtered_device(cvttmi_context *ctx, void *d_pyramid, size_t pyramidBytes, const void *d_image, uint32_t width,
                                          uint32_t height, size_t rowPitchBytes, int pixelFormat, uint32_t levels, uint32_t filter,
                                          void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        const size_t texel = mipTexelBytes(pixelFormat);
        if (!d_image || texel == 0 || width == 0 || height == 0 || rowPitchBytes < (size_t)width * texel || (rowPitchBytes % texel) != 0 ||
            levels == 0 || levels > cvttmi_mip_level_count(width, height))
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        cvttmi_mip_level table[kMaxMipLevels + 1];
        if (cvttmi_mip_layout(width, height, pixelFormat, 16, levels, table) != CVTTMI_OK || (levels > 1 && !d_pyramid))
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (pyramidBytes < table[levels].byteOffset)
            return fail(ctx, CVTTMI_E_INVALID, "pyramid buffer smaller than cvttmi_mip_layout asks for");
        if (!alignedTo(d_image, texel) || !alignedTo(d_pyramid, texel))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        if (!mipFilterFits(pixelFormat, filter))
            return fail(ctx, CVTTMI_E_INVALID, kMipFilterText);
        if (levels == 1)
            return CVTTMI_OK;
        // a texture of one layer: no layer stride is read, so the pyramid may end where its last level ends
        return withDevice(ctx, [&] {
            return queueMips(ctx, static_cast<uint8_t *>(d_pyramid), 0, table, static_cast<const uint8_t *>(d_image), rowPitchBytes, 0, pixelFormat,
                             levels, 1, filter, static_cast<hipStream_t>(hipStream));
        });
    }

    // ---- texture arrays and cube maps (cvtt_mi355x.h, "texture arrays and cube maps") ----
    // One layer's table (cvttmi_mip_layout: kMaxMipLevels + 1 entries) and the sizes of all layers; false = invalid.
    static bool textureSizes(uint32_t width, uint32_t height, int pixelFormat, uint32_t bytesPerBlock, uint32_t levels, uint32_t layers,
                             int order, cvttmi_mip_level *table, cvttmi_texture_sizes *sizes)
    {
        if (layers == 0 || (order != CVTTMI_ORDER_LAYER_MAJOR && order != CVTTMI_ORDER_LEVEL_MAJOR) ||
            cvttmi_mip_layout(width, height, pixelFormat, bytesPerBlock, levels, table) != CVTTMI_OK)
            return false;
        const cvttmi_mip_level &end = table[levels];
        cvttmi_texture_sizes s;
        if (end.byteOffset > SIZE_MAX - 255)
            return false;
        s.pyramidLayerBytes = (end.byteOffset + 255) / 256 * 256;
        s.tilesPerLayer = end.firstTile;
        s.blocksPerLayer = end.firstBlock;
        if (__builtin_mul_overflow(s.pyramidLayerBytes, (size_t)layers, &s.pyramidBytes) ||
            __builtin_mul_overflow(s.tilesPerLayer, (size_t)layers, &s.tiles) || __builtin_mul_overflow(s.blocksPerLayer, (size_t)layers, &s.blocks) ||
            s.tiles > 0xffffffffull || s.blocks > 0xffffffffull)
            return false;
        // the work space: [pyramids | tiles | padded packed blocks]; the first two parts are multiples of 256 bytes
        const size_t tileBytes = s.tiles * 16 * mipTexelBytes(pixelFormat), packedBytes = s.tiles * bytesPerBlock; // (tiles < 2^32)
        if (__builtin_add_overflow(s.pyramidBytes, tileBytes, &s.workBytes) || __builtin_add_overflow(s.workBytes, packedBytes, &s.workBytes))
            return false;
        *sizes = s;
        return true;
    }

    int cvttmi_texture_layout(uint32_t width, uint32_t height, int pixelFormat, uint32_t bytesPerBlock, uint32_t levels, uint32_t layers,
                              int order, cvttmi_texture_sizes *out)
    {
        cvttmi_mip_level table[kMaxMipLevels + 1];
        cvttmi_texture_sizes sizes;
        if (!out || !textureSizes(width, height, pixelFormat, bytesPerBlock, levels, layers, order, table, &sizes))
            return CVTTMI_E_INVALID;
        *out = sizes;
        return CVTTMI_OK;
    }

    int cvttmi_texture_subresource(uint32_t width, uint32_t height, int pixelFormat, uint32_t bytesPerBlock, uint32_t levels, uint32_t layers,
                                   int order, uint32_t layer, uint32_t level, size_t *firstBlock, size_t *blockCount)
    {
        cvttmi_mip_level table[kMaxMipLevels + 1];
        cvttmi_texture_sizes sizes;
        if (!textureSizes(width, height, pixelFormat, bytesPerBlock, levels, layers, order, table, &sizes) || layer >= layers || level >= levels)
            return CVTTMI_E_INVALID;
        const cvttmi_mip_level &L = table[level];
        if (firstBlock)
            *firstBlock = order == CVTTMI_ORDER_LEVEL_MAJOR ? (size_t)layers * L.firstBlock + (size_t)layer * L.blockCount
                                                            : (size_t)layer * sizes.blocksPerLayer + L.firstBlock;
        if (blockCount)
            *blockCount = L.blockCount;
        return CVTTMI_OK;
    }

    // the images of a texture as the two entries below take them: NULL = fine, else what is wrong
    static const char *textureImagesWrong(const void *d_images, uint32_t width, uint32_t height, size_t rowPitchBytes, size_t layerPitchBytes,
                                          size_t texel, uint32_t layers)
    {
        size_t imageBytes, allBytes;
        if (!d_images || texel == 0 || width == 0 || height == 0 || layers == 0 || rowPitchBytes < (size_t)width * texel || (rowPitchBytes % texel) != 0)
            return "invalid argument";
        if (__builtin_mul_overflow(rowPitchBytes, (size_t)height, &imageBytes) || layerPitchBytes < imageBytes || (layerPitchBytes % texel) != 0 ||
            __builtin_mul_overflow(layerPitchBytes, (size_t)layers, &allBytes))
            return "layerPitchBytes must be a multiple of the texel and at least height x rowPitchBytes";
        return NULL;
    }

    int cvttmi_build_mips_array_device(cvttmi_context *ctx, void *d_pyramids, size_t pyramidBytes, const void *d_images, uint32_t width,
                                       uint32_t height, size_t rowPitchBytes, size_t layerPitchBytes, int pixelFormat, uint32_t levels,
                                       uint32_t layers, uint32_t filter, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        const size_t texel = mipTexelBytes(pixelFormat);
        if (const char *wrong = textureImagesWrong(d_images, width, height, rowPitchBytes, layerPitchBytes, texel, layers))
            return fail(ctx, CVTTMI_E_INVALID, wrong);
        cvttmi_mip_level table[kMaxMipLevels + 1];
        cvttmi_texture_sizes sizes;
        if (!textureSizes(width, height, pixelFormat, 16, levels, layers, CVTTMI_ORDER_LAYER_MAJOR, table, &sizes) || (levels > 1 && !d_pyramids))
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (pyramidBytes < sizes.pyramidBytes)
            return fail(ctx, CVTTMI_E_INVALID, "pyramid buffer smaller than cvttmi_texture_layout asks for");
        if (!alignedTo(d_images, texel) || !alignedTo(d_pyramids, texel))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        if (!mipFilterFits(pixelFormat, filter))
            return fail(ctx, CVTTMI_E_INVALID, kMipFilterText);
        if (levels == 1)
            return CVTTMI_OK;
        return withDevice(ctx, [&] {
            return queueMips(ctx, static_cast<uint8_t *>(d_pyramids), sizes.pyramidLayerBytes, table, static_cast<const uint8_t *>(d_images),
                             rowPitchBytes, layerPitchBytes, pixelFormat, levels, layers, filter, static_cast<hipStream_t>(hipStream));
        });
    }

    int cvttmi_encode_texture_device(cvttmi_context *ctx, int format, void *d_out, size_t outBytes, const void *d_images, uint32_t width,
                                     uint32_t height, size_t rowPitchBytes, size_t layerPitchBytes, uint32_t layers, uint32_t levels,
                                     uint32_t filter, int order, const cvttmi_options *options, const cvttmi_bc7_plan *plan,
                                     const cvttmi_options *allocOptions, void *d_work, size_t workBytes, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        size_t bcBytes = 0, tileBytes = 0;
        const CvttTextureFormat *row = formatInfo(format, &bcBytes, &tileBytes);
        if (!row || row->image == kCvttNoImage) // (R11: no image form)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        // the images a format is built from are of its row's kind, the snorm class averaging them as int8
        const int pixelFormat = row->cls == kCvttSnorm8 ? CVTTMI_PIXELS_RGBA8_SNORM : row->image;
        const size_t texel = mipTexelBytes(pixelFormat);
        if (!d_out || !d_work || !options || (!plan && encoderTakesPlan(format)))
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (const char *wrong = textureImagesWrong(d_images, width, height, rowPitchBytes, layerPitchBytes, texel, layers))
            return fail(ctx, CVTTMI_E_INVALID, wrong);
        cvttmi_mip_level table[kMaxMipLevels + 1];
        cvttmi_texture_sizes sizes;
        if (!textureSizes(width, height, pixelFormat, static_cast<uint32_t>(bcBytes), levels, layers, order, table, &sizes))
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (outBytes != sizes.blocks * bcBytes)
            return fail(ctx, CVTTMI_E_INVALID, "outBytes is not the texture's blocks x bytes per block (cvttmi_texture_layout)");
        if (workBytes < sizes.workBytes)
            return fail(ctx, CVTTMI_E_INVALID, "work space smaller than cvttmi_texture_layout asks for");
        if (!alignedTo(d_out, bcBytes) || !alignedTo(d_images, texel) || (reinterpret_cast<uintptr_t>(d_work) & 255u) != 0)
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        if (!mipFilterFits(pixelFormat, filter))
            return fail(ctx, CVTTMI_E_INVALID, kMipFilterText);

        uint8_t *pyramids = static_cast<uint8_t *>(d_work);
        uint8_t *tiles = pyramids + sizes.pyramidBytes;
        uint8_t *packed = tiles + sizes.tiles * tileBytes;
        static_assert(kCvttDecodeLevels >= kMaxMipLevels, "the level table of the texture kernels");
        CvttTextureLevels args;
        memset(&args, 0, sizeof(args));
        for (uint32_t l = 0; l < levels; l++)
        {
            CvttTextureLevel &L = args.level[l];
            L.image = l == 0 ? static_cast<const uint8_t *>(d_images) : pyramids + table[l].byteOffset;
            L.pitch = l == 0 ? rowPitchBytes : table[l].rowPitchBytes;
            L.layerStride = l == 0 ? layerPitchBytes : sizes.pyramidLayerBytes;
            L.width = table[l].width;
            L.height = table[l].height;
            L.blocksPerRow = static_cast<uint32_t>(((uint64_t)table[l].width + 3) / 4);
            L.tilesPerRow = static_cast<uint32_t>(((uint64_t)L.blocksPerRow + 7) / 8 * 8);
            L.firstTile = static_cast<uint32_t>(table[l].firstTile);
            L.firstBlock = static_cast<uint32_t>(table[l].firstBlock);
            L.blockCount = static_cast<uint32_t>(table[l].blockCount);
        }
        args.count = levels;
        args.layers = layers;
        args.tilesPerLayer = static_cast<uint32_t>(sizes.tilesPerLayer);
        args.blocksPerLayer = static_cast<uint32_t>(sizes.blocksPerLayer);
        args.levelMajor = order == CVTTMI_ORDER_LEVEL_MAJOR;

        hipStream_t stream = static_cast<hipStream_t>(hipStream);
        return withDevice(ctx, [&] {
            return timed(ctx, stream, [&] {
                if (levels > 1)
                {
                    const int rc = queueMips(ctx, pyramids, sizes.pyramidLayerBytes, table, static_cast<const uint8_t *>(d_images), rowPitchBytes,
                                             layerPitchBytes, pixelFormat, levels, layers, filter, stream);
                    if (rc != CVTTMI_OK)
                        return rc;
                }
                hipError_t e = cvttmi_launch_tile_chain(&args, tiles, static_cast<uint32_t>(texel), stream);
                if (e != hipSuccess)
                    return fail(ctx, CVTTMI_E_HIP, "chain tile kernel launch", e);
                // one search over every tile; a count beyond one call's limit is cut at a group boundary (the limit is a multiple of 8)
                static_assert(kMaxLaunchBlocks % 8 == 0, "groups of eight");
                for (size_t first = 0; first < sizes.tiles; first += kMaxLaunchBlocks)
                {
                    const size_t n = sizes.tiles - first < kMaxLaunchBlocks ? sizes.tiles - first : kMaxLaunchBlocks;
                    const int rc = encodeBlocks(ctx, format, options, plan, allocOptions, packed + first * bcBytes, tiles + first * tileBytes, n, stream);
                    if (rc != CVTTMI_OK)
                        return rc;
                }
                e = cvttmi_launch_compact_chain(&args, packed, d_out, static_cast<uint32_t>(bcBytes), stream);
                return e == hipSuccess ? CVTTMI_OK : fail(ctx, CVTTMI_E_HIP, "chain compact kernel launch", e);
            });
        });
    }

    // ---- resize (cvtt_mi355x.h, "resize") ----
    namespace
    {
        const uint32_t kResizeMaxSize = 65535;
        const uint32_t kResizeBox = 0; // kernel code 0 of the resize calls

        // the weight functions of the mip kernels (cvtt_mi355x.h, "mip kernels and wrap modes"), in double precision
        double resizeSinc(double x) { return x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x); }
        double resizeI0(double x)
        {
            double total = 1.0, term = 1.0;
            for (int k = 1; term > 1e-17 * total; k++)
            {
                const double f = x / (2.0 * k);
                term *= pow(f, 2); // (pow: the restatement's ** 2, bit for bit)
                total += term;
            }
            return total;
        }
        double resizeWeight(uint32_t code, double t)
        {
            const double a = fabs(t);
            if (code == 1)
                return a < 1.0 ? 1.0 - a : 0.0;
            if (code == 2)
            {
                const double b = 1.0 / 3.0, c = 1.0 / 3.0;
                if (a < 1.0)
                    return ((12 - 9 * b - 6 * c) * pow(a, 3) + (-18 + 12 * b + 6 * c) * pow(a, 2) + (6 - 2 * b)) / 6.0;
                if (a < 2.0)
                    return ((-b - 6 * c) * pow(a, 3) + (6 * b + 30 * c) * pow(a, 2) + (-12 * b - 48 * c) * a + (8 * b + 24 * c)) / 6.0;
                return 0.0;
            }
            if (a >= 3.0)
                return 0.0;
            if (code == 3)
                return resizeSinc(t) * resizeSinc(t / 3.0);
            const double u = t / 3.0;
            return resizeSinc(t) * resizeI0(4.0 * sqrt(1.0 - pow(u, 2))) / resizeI0(4.0);
        }

        int64_t floorDiv(int64_t a, int64_t b) // b > 0
        {
            return a >= 0 ? a / b : -((-a + b - 1) / b);
        }

        // twice the radius of a kernel code (box: 1 = twice a half); 0 = no such kernel
        uint32_t resizeRadius2(uint32_t code)
        {
            static const uint32_t r2[CVTT_MIP_KERNELS + 1] = {1, 2, 4, 6, 6};
            return code <= CVTT_MIP_KERNELS ? r2[code] : 0;
        }
        // the filter word of the resize calls: rule (one that RGBA8, which takes them all, takes) | kernel (0 = box) | at most one wrap
        // flag, or the word of RGBA16F: the plain rule | kernel | wrap | one range flag; false = not such a word
        bool resizeFilterOk(const FilterWord &f)
        {
            return resizeRadius2(f.code) != 0 && oneWrapAtMost(f.wrap) &&
                   kernelRuleFits(f.range ? CVTTMI_PIXELS_RGBA16F : CVTTMI_PIXELS_RGBA8, f.rule, f.range);
        }
        uint32_t resizeTapCount(uint32_t src, uint32_t dst, uint32_t code)
        {
            const uint64_t big = src > dst ? src : dst;
            return static_cast<uint32_t>(code == kResizeBox ? (big + dst - 1) / dst + 1 : (resizeRadius2(code) * big + dst - 1) / dst);
        }
        int32_t resizeFirst(uint32_t src, uint32_t dst, uint32_t code, uint32_t x)
        {
            const int64_t big = src > dst ? src : dst;
            const int64_t L = (2 * (int64_t)x + 1) * src - dst - (int64_t)resizeRadius2(code) * big;
            return static_cast<int32_t>(code == kResizeBox ? floorDiv(L + dst, 2 * (int64_t)dst) : floorDiv(L, 2 * (int64_t)dst) + 1);
        }

        // The one owner of the rule: the tables of one axis.  Weight k of output x goes to weights[x * strideX + k * strideK].  Rows
        // repeat: with g = gcd(src, dst), output x + dst / g sees the source exactly as x does, src / g texels further on, so only
        // the first dst / g rows are computed.  false = the guard on the int32 sums refuses the table.
        bool resizeTable(uint32_t src, uint32_t dst, uint32_t code, int16_t *weights, size_t strideX, size_t strideK, int32_t *first)
        {
            const uint32_t n = resizeTapCount(src, dst, code);
            const int64_t big = src > dst ? src : dst;
            uint32_t g = src, b = dst;
            while (b)
            {
                const uint32_t t = g % b;
                g = b;
                b = t;
            }
            const uint32_t period = dst / g, shift = src / g;
            std::vector<double> w(n);
            std::vector<int32_t> q(n);
            int64_t P = 0;
            for (uint32_t x = 0; x < dst && x < period; x++)
            {
                const int64_t f = resizeFirst(src, dst, code, x);
                const int64_t centre = (2 * (int64_t)x + 1) * src - dst; // in units of 1 / (2 dst)
                if (src == dst)
                {
                    // an image resized to its own size is itself: what the formulas below give for every kernel but Mitchell,
                    // whose K(0) = 8/9 would blur it
                    for (uint32_t k = 0; k < n; k++)
                        q[k] = f + k == (int64_t)x ? 16384 : 0;
                }
                else if (code == kResizeBox)
                {
                    const int64_t lo = centre - big, hi = centre + big;
                    for (uint32_t k = 0; k < n; k++)
                    {
                        const int64_t a0 = 2 * (int64_t)dst * (f + k) - dst, a1 = a0 + 2 * (int64_t)dst;
                        const int64_t o = (a1 < hi ? a1 : hi) - (a0 > lo ? a0 : lo);
                        q[k] = static_cast<int32_t>((2 * 16384 * (o > 0 ? o : 0) + 2 * big) / (4 * big));
                    }
                }
                else
                {
                    double W = 0.0;
                    for (uint32_t k = 0; k < n; k++)
                    {
                        w[k] = resizeWeight(code, (double)(2 * (int64_t)dst * (f + k) - centre) / (double)(2 * big));
                        W += w[k];
                    }
                    for (uint32_t k = 0; k < n; k++)
                        q[k] = static_cast<int32_t>(floor(16384.0 * (w[k] / W) + 0.5));
                }
                // what is missing to 16384 goes to the taps that hold the row's largest value, the lowest index first
                int64_t sum = 0;
                int32_t top = q[0];
                for (uint32_t k = 0; k < n; k++)
                {
                    sum += q[k];
                    top = q[k] > top ? q[k] : top;
                }
                uint32_t tops = 0;
                for (uint32_t k = 0; k < n; k++)
                    tops += q[k] == top;
                const int64_t rest = 16384 - sum, each = rest / (int64_t)tops;
                int64_t left = rest - each * tops, pos = 0;
                for (uint32_t k = 0; k < n; k++)
                {
                    int64_t v = q[k];
                    if (q[k] == top)
                    {
                        v += each + left;
                        left = 0;
                    }
                    if (v < -32768 || v > 32767)
                        return false;
                    pos += v > 0 ? v : 0;
                    weights[x * strideX + k * strideK] = static_cast<int16_t>(v);
                }
                P = pos > P ? pos : P;
                first[x] = static_cast<int32_t>(f);
            }
            for (uint32_t x = period; x < dst; x++)
            {
                for (uint32_t k = 0; k < n; k++)
                    weights[x * strideX + k * strideK] = weights[(x - period) * strideX + k * strideK];
                first[x] = first[x - period] + static_cast<int32_t>(shift);
            }
            // int32 in both passes, the sRGB values (T <= 65535) being the largest: |h| <= 65535 P, |s| <= max |h'| x sum |q|
            return 65535 * P < ((int64_t)1 << 31) && ((65535 * P + 8192) >> 14) * (2 * P - 16384) < ((int64_t)1 << 31);
        }

        size_t up256(size_t v) { return (v + 255) / 256 * 256; }

        // where a call's tables lie in its work space, and what else the work space holds
        struct ResizePlan
        {
            FilterWord f;
            uint32_t nx, ny, fusedRows; // fusedRows: 0 = two launches through the intermediate
            size_t wx, fx, wy, fy, tableBytes, workBytes;
        };
        const char *const kResizeFilterText =
            "resize filter: the plain rule, SRGB or NORMAL (RGBA8_SNORM: not SRGB) | kernel 0 (box) or a CVTTMI_MIP_KERNEL_* | at most one "
            "CVTTMI_MIP_WRAP_* flag; RGBA8 or RGBA8_SNORM texels, or RGBA16F texels with the plain rule and exactly one CVTTMI_MIP_HDR_* flag "
            "(a flag goes with nothing else)";
        // NULL = fine, else what is wrong
        const char *resizePlan(uint32_t srcW, uint32_t srcH, uint32_t dstW, uint32_t dstH, int pixelFormat, uint32_t filter, uint32_t layers,
                               ResizePlan *plan)
        {
            if (srcW == 0 || srcH == 0 || dstW == 0 || dstH == 0 || layers == 0 || (srcW | srcH | dstW | dstH | layers) > kResizeMaxSize)
                return "resize: sizes and layers are 1 .. 65535";
            ResizePlan p;
            p.f = splitFilter(filter);
            if (!resizeFilterOk(p.f) || !kernelRuleFits(pixelFormat, p.f.rule, p.f.range))
                return kResizeFilterText;
            const uint32_t code = p.f.code, rule = p.f.rule;
            p.nx = resizeTapCount(srcW, dstW, code);
            p.ny = resizeTapCount(srcH, dstH, code);
            p.wx = 0;
            p.fx = p.wx + up256((size_t)dstW * p.nx * sizeof(int16_t));
            p.wy = p.fx + up256((size_t)dstW * sizeof(int32_t));
            p.fy = p.wy + up256((size_t)dstH * p.ny * sizeof(int16_t));
            p.tableBytes = p.fy + up256((size_t)dstH * sizeof(int32_t));
            std::vector<int32_t> first(dstH);
            for (uint32_t y = 0; y < dstH; y++)
                first[y] = resizeFirst(srcH, dstH, code, y);
            p.fusedRows = cvttmi_resize_fused_rows(pixelFormat, rule, first.data(), dstH, p.ny);
            p.workBytes = p.tableBytes + (p.fusedRows ? 0 : (size_t)layers * srcH * dstW * cvttmi_resize_entry_bytes(pixelFormat, rule)); // (below 2^52)
            *plan = p;
            return NULL;
        }
    } // namespace

    int cvttmi_resize_taps(uint32_t src, uint32_t dst, uint32_t filter, int16_t *weights, int32_t *first, uint32_t *tapsPerRow)
    {
        const FilterWord f = splitFilter(filter);
        if (src == 0 || dst == 0 || src > kResizeMaxSize || dst > kResizeMaxSize || !resizeFilterOk(f) || !tapsPerRow || (weights && !first))
            return CVTTMI_E_INVALID;
        *tapsPerRow = resizeTapCount(src, dst, f.code);
        if (!weights)
            return CVTTMI_OK;
        return resizeTable(src, dst, f.code, weights, *tapsPerRow, 1, first) ? CVTTMI_OK : CVTTMI_E_INVALID;
    }

    int cvttmi_resize_work_bytes(uint32_t srcW, uint32_t srcH, uint32_t dstW, uint32_t dstH, int pixelFormat, uint32_t filter, uint32_t layers,
                                 size_t *workBytes)
    {
        ResizePlan plan;
        if (!workBytes || resizePlan(srcW, srcH, dstW, dstH, pixelFormat, filter, layers, &plan))
            return CVTTMI_E_INVALID;
        *workBytes = plan.workBytes;
        return CVTTMI_OK;
    }

    int cvttmi_resize_launches(uint32_t srcW, uint32_t srcH, uint32_t dstW, uint32_t dstH, int pixelFormat, uint32_t filter, uint32_t *launches)
    {
        ResizePlan plan;
        if (!launches || resizePlan(srcW, srcH, dstW, dstH, pixelFormat, filter, 1, &plan))
            return CVTTMI_E_INVALID;
        *launches = plan.fusedRows ? 1 : 2;
        return CVTTMI_OK;
    }

    int cvttmi_resize_image_device(cvttmi_context *ctx, void *d_dst, uint32_t dstW, uint32_t dstH, size_t dstRowPitchBytes, size_t dstLayerPitchBytes,
                                   const void *d_src, uint32_t srcW, uint32_t srcH, size_t srcRowPitchBytes, size_t srcLayerPitchBytes,
                                   int pixelFormat, uint32_t layers, uint32_t filter, void *d_work, size_t workBytes, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        ResizePlan plan;
        if (const char *wrong = resizePlan(srcW, srcH, dstW, dstH, pixelFormat, filter, layers, &plan))
            return fail(ctx, CVTTMI_E_INVALID, wrong);
        if (!d_work)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        const size_t texel = mipTexelBytes(pixelFormat); // (the plan has passed the kind)
        if (const char *wrong = textureImagesWrong(d_src, srcW, srcH, srcRowPitchBytes, srcLayerPitchBytes, texel, layers))
            return fail(ctx, CVTTMI_E_INVALID, wrong);
        if (const char *wrong = textureImagesWrong(d_dst, dstW, dstH, dstRowPitchBytes, dstLayerPitchBytes, texel, layers))
            return fail(ctx, CVTTMI_E_INVALID, wrong);
        if (workBytes < plan.workBytes)
            return fail(ctx, CVTTMI_E_INVALID, "work space smaller than cvttmi_resize_work_bytes asks for");
        if (!alignedTo(d_src, texel) || !alignedTo(d_dst, texel) || (reinterpret_cast<uintptr_t>(d_work) & 255u) != 0)
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        const uint32_t code = plan.f.code, tablesOf = filter & ~(plan.f.wrap | plan.f.range); // (the tables depend on neither the wrap nor the range)
        hipStream_t stream = static_cast<hipStream_t>(hipStream);
        return withDevice(ctx, [&] {
            // the slot that holds these tables already, or the next of the ring
            cvttmi_context::ResizeSlot *slot = NULL;
            for (int i = 0; i < cvttmi_context::kResizeSlots && !slot; i++)
            {
                cvttmi_context::ResizeSlot &s = ctx->resizeSlot[i];
                if (s.valid && s.srcW == srcW && s.srcH == srcH && s.dstW == dstW && s.dstH == dstH && s.filter == tablesOf)
                    slot = &s;
            }
            const bool held = slot != NULL;
            if (!slot)
            {
                slot = &ctx->resizeSlot[ctx->nextResizeSlot];
                ctx->nextResizeSlot = (ctx->nextResizeSlot + 1) % cvttmi_context::kResizeSlots;
            }
            hipError_t e;
            // a slot's one event stands for its latest copy: before the slot is rewritten, and before a copy on another stream
            // takes the event over, that copy has finished
            if (slot->inFlight && (!held || slot->stream != stream))
            {
                if ((e = hipEventSynchronize(slot->ev)) != hipSuccess)
                    return fail(ctx, CVTTMI_E_HIP, "hipEventSynchronize(resize tables)", e);
                slot->inFlight = false;
            }
            if (!held)
            {
                slot->valid = false;
                if ((e = slot->pinned.reserve(plan.tableBytes)) != hipSuccess) // (the copy that last read it has finished, above)
                    return fail(ctx, CVTTMI_E_HIP, "hipHostMalloc(resize tables)", e);
                if ((e = slot->ev.create(hipEventDisableTiming)) != hipSuccess)
                    return fail(ctx, CVTTMI_E_HIP, "hipEventCreate(resize tables)", e);
                uint8_t *t = slot->pinned.as<uint8_t>();
                memset(t, 0, plan.tableBytes);
                // columns tap-major (the lanes of a wave are neighbouring columns), rows row-major (a wave is in one row)
                if (!resizeTable(srcW, dstW, code, reinterpret_cast<int16_t *>(t + plan.wx), 1, dstW, reinterpret_cast<int32_t *>(t + plan.fx)) ||
                    !resizeTable(srcH, dstH, code, reinterpret_cast<int16_t *>(t + plan.wy), plan.ny, 1, reinterpret_cast<int32_t *>(t + plan.fy)))
                    return fail(ctx, CVTTMI_E_INVALID, "resize: the weight table of these sizes does not keep the sums inside int32");
                slot->srcW = srcW;
                slot->srcH = srcH;
                slot->dstW = dstW;
                slot->dstH = dstH;
                slot->filter = tablesOf;
                slot->valid = true;
            }
            return timed(ctx, stream, [&] {
                uint8_t *work = static_cast<uint8_t *>(d_work);
                hipError_t e2 = hipMemcpyAsync(work, slot->pinned.get(), plan.tableBytes, hipMemcpyHostToDevice, stream);
                if (e2 != hipSuccess)
                    return fail(ctx, CVTTMI_E_HIP, "hipMemcpyAsync(resize tables)", e2);
                slot->stream = stream;
                slot->inFlight = hipEventRecord(slot->ev, stream) == hipSuccess;
                if (!slot->inFlight)
                    (void)hipStreamSynchronize(stream); // (no event to wait for later: the copy ends here)
                e2 = cvttmi_launch_resize(d_src, srcRowPitchBytes, srcLayerPitchBytes, srcW, srcH, d_dst, dstRowPitchBytes, dstLayerPitchBytes, dstW,
                                          dstH, layers, pixelFormat, plan.f.rule, plan.f.wrap, plan.f.range, reinterpret_cast<const int16_t *>(work + plan.wx),
                                          reinterpret_cast<const int32_t *>(work + plan.fx), plan.nx, reinterpret_cast<const int16_t *>(work + plan.wy),
                                          reinterpret_cast<const int32_t *>(work + plan.fy), plan.ny, work + plan.tableBytes, plan.fusedRows, stream);
                return e2 == hipSuccess ? CVTTMI_OK : fail(ctx, CVTTMI_E_HIP, "resize kernel launch", e2);
            });
        });
    }
}
