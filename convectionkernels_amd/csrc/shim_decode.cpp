// Packed blocks back into texels (cvtt_mi355x.h: decoding, "decoding into images", the error measure): the decode, decode-to-image,
// decode-mips and measure entries, and cvttmi_psnr.
#include "shim_internal.h"

#include <math.h>

using namespace cvtt_shim;

namespace
{
    // packed blocks -> the decoded layout of `format`
    auto decodeFormatBody(cvttmi_context *ctx, int format)
    {
        return [=](void *dOut, const void *dIn, size_t numBlocks, hipStream_t stream) -> int {
            const hipError_t e = cvttmi_launch_decode(dIn, dOut, static_cast<uint32_t>(numBlocks), format, ctx->tables(), stream);
            return e == hipSuccess ? CVTTMI_OK : fail(ctx, CVTTMI_E_HIP, "decode kernel launch", e);
        };
    }

    // The image a format decodes into and is measured against: bytes of its texel (a sixteenth of its decoded block) when
    // `pixels` is the kind of the format's row, else -- and for R11, which has no image form -- 0.  bcBytes: bytes per packed block.
    size_t imageTexelBytes(int format, int pixels, size_t *bcBytes)
    {
        const CvttTextureFormat *row = formatInfo(format, bcBytes);
        return row && row->image != kCvttNoImage && pixels == row->image ? row->texBytes / 16u : 0u;
    }

    const size_t kMeasureLaunch = (size_t)1 << 24; // blocks per measure launch (decode_kernel.hip)

    // The measure on device pointers: launches of at most 2^24 blocks, each adding into d_totals in order.  source 0: blocks
    // (texels = 16 per block), 1 + CVTTMI_PIXELS_*: an RGBA8 (1) / RGBA16F (2) image of width x height.
    int measureLaunches(cvttmi_context *ctx, int format, const void *dBc, const void *dSource, int source, uint32_t width, uint32_t height,
                        size_t pitch, size_t numBlocks, void *dBlockError, cvttmi_error_totals *dTotals, hipStream_t stream)
    {
        size_t bcBytes = 0, texBytes = 0;
        formatInfo(format, &bcBytes, &texBytes, NULL);
        hipError_t e;
        if ((e = ctx->dMeasureSlab.reserve(kMeasureLaunch / 256 * 4 * 8)) != hipSuccess)
            return fail(ctx, CVTTMI_E_HIP, "hipMalloc(measure slab)", e);
        orderAfterPrevious(ctx, stream);
        // image: texels inside width x height of the blocks before block b (row-major, ceil(width / 4) blocks per row)
        const size_t blocksPerRow = (width + 3) / 4;
        auto texelsBefore = [&](size_t b) -> uint64_t {
            const size_t row = b / blocksPerRow, col = b % blocksPerRow;
            const uint64_t rowsAbove = 4 * (uint64_t)row < height ? 4 * (uint64_t)row : height;
            const uint64_t rowHeight = height - rowsAbove < 4 ? height - rowsAbove : 4;
            const uint64_t cols = 4 * (uint64_t)col < width ? 4 * (uint64_t)col : width;
            return (uint64_t)width * rowsAbove + cols * rowHeight;
        };
        for (size_t first = 0; first < numBlocks || first == 0; first += kMeasureLaunch) // (0 blocks: one launch writes empty totals)
        {
            const size_t n = (numBlocks - first) < kMeasureLaunch ? (numBlocks - first) : kMeasureLaunch;
            const uint64_t texels = source == 0 ? 16 * (uint64_t)n : texelsBefore(first + n) - texelsBefore(first);
            const void *src = source == 0 ? static_cast<const void *>(static_cast<const uint8_t *>(dSource) + first * texBytes) : dSource;
            void *blockErr = dBlockError ? static_cast<void *>(static_cast<uint8_t *>(dBlockError) + first * 4) : NULL;
            e = cvttmi_launch_measure(static_cast<const uint8_t *>(dBc) + first * bcBytes, src, source, width, height, pitch, first,
                                      static_cast<uint32_t>(n), format, blockErr, ctx->dMeasureSlab.get(), dTotals, first != 0, texels, ctx->tables(), stream);
            if (e != hipSuccess)
            {
                if (first != 0)
                    (void)hipStreamSynchronize(stream);
                return fail(ctx, CVTTMI_E_HIP, "measure kernel launch", e);
            }
        }
        markLaunch(ctx, stream);
        return CVTTMI_OK;
    }
}

extern "C"
{
    int cvttmi_decode_device(cvttmi_context *ctx, int format, void *d_out, const void *d_bc, size_t numBlocks, void *hipStream)
    {
        size_t bcBytes = 16, texBytes = 64;
        const bool ok = formatInfo(format, &bcBytes, &texBytes, NULL);
        return onDevice(ctx, d_out, d_bc, numBlocks, ok, bcBytes, texBytes, hipStream, decodeFormatBody(ctx, format));
    }
    int cvttmi_decode(cvttmi_context *ctx, int format, void *out, const uint8_t *bc, size_t numBlocks)
    {
        size_t bcBytes = 16, texBytes = 64;
        const bool ok = formatInfo(format, &bcBytes, &texBytes, NULL);
        return onHost(ctx, out, bc, numBlocks, ok, bcBytes, texBytes, false, decodeFormatBody(ctx, format));
    }

    int cvttmi_decode_bc7_device(cvttmi_context *ctx, void *d_blocks, const void *d_bc, size_t numBlocks, void *hipStream)
    { return cvttmi_decode_device(ctx, CVTTMI_FMT_BC7, d_blocks, d_bc, numBlocks, hipStream); }
    int cvttmi_decode_bc6h_device(cvttmi_context *ctx, void *d_blocksF16, const void *d_bc, size_t numBlocks, int isSigned, void *hipStream)
    { return cvttmi_decode_device(ctx, isSigned ? CVTTMI_FMT_BC6HS : CVTTMI_FMT_BC6HU, d_blocksF16, d_bc, numBlocks, hipStream); }
    int cvttmi_decode_bc7(cvttmi_context *ctx, uint8_t *blocks, const uint8_t *bc, size_t numBlocks)
    { return cvttmi_decode(ctx, CVTTMI_FMT_BC7, blocks, bc, numBlocks); }
    int cvttmi_decode_bc6h(cvttmi_context *ctx, uint8_t *blocksF16, const uint8_t *bc, size_t numBlocks, int isSigned)
    { return cvttmi_decode(ctx, isSigned ? CVTTMI_FMT_BC6HS : CVTTMI_FMT_BC6HU, blocksF16, bc, numBlocks); }

    int cvttmi_measure_error_device(cvttmi_context *ctx, int format, const void *d_bc, const void *d_source, size_t numBlocks,
                                    void *d_blockError, cvttmi_error_totals *d_totals, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        size_t bcBytes = 0, texBytes = 0;
        if (!formatInfo(format, &bcBytes, &texBytes, NULL) || !d_bc || !d_source || !d_totals || (numBlocks % 8) != 0 || numBlocks > kMaxLaunchBlocks)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (!alignedTo(d_bc, bcBytes) || !alignedTo(d_source, texBytes) || !alignedTo(d_blockError, 4) || !alignedTo(d_totals, 8))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        hipStream_t stream = static_cast<hipStream_t>(hipStream);
        return withDevice(ctx, [&] {
            return timed(ctx, stream, [&] { return measureLaunches(ctx, format, d_bc, d_source, 0, 0, 0, 0, numBlocks, d_blockError, d_totals, stream); });
        });
    }

    // host buffers: chunks of 2^17 blocks through the context's measure buffers, each chunk's totals added on the host in order
    int cvttmi_measure_error(cvttmi_context *ctx, int format, const uint8_t *bc, const void *source, size_t numBlocks,
                             void *blockError, cvttmi_error_totals *totals)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        size_t bcBytes = 0, texBytes = 0;
        uint32_t mask = 0;
        if (!formatInfo(format, &bcBytes, &texBytes, &mask) || !bc || !source || !totals || (numBlocks % 8) != 0)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        return withDevice(ctx, [&]() -> int {
            const size_t chunk = (size_t)1 << 17;
            // one allocation: [packed | sources | per-block values | totals], each part 256-byte aligned
            const size_t offSrc = chunk * bcBytes, offErr = offSrc + chunk * texBytes, offTot = offErr + chunk * 4;
            const size_t need = offTot + 256;
            hipError_t e;
            if (ctx->dMeasureHost.bytes() < need)
            {
                if (ctx->dMeasureHost)
                    (void)hipStreamSynchronize(ctx->stream()); // the previous call's copies and launches ran there
                if ((e = ctx->dMeasureHost.reserve(need)) != hipSuccess)
                    return fail(ctx, CVTTMI_E_HIP, "hipMalloc(measure buffers)", e);
            }
            uint8_t *dBase = ctx->dMeasureHost.as<uint8_t>();
            uint8_t *dBc = dBase, *dSrc = dBase + offSrc, *dErr = blockError ? dBase + offErr : NULL;
            cvttmi_error_totals *dTot = reinterpret_cast<cvttmi_error_totals *>(dBase + offTot);
            cvttmi_error_totals sum;
            memset(&sum, 0, sizeof(sum));
            sum.channelMask = mask;
            sum.format = format;
            hipStream_t stream = ctx->stream();
            int rc = CVTTMI_OK;
            for (size_t first = 0; rc == CVTTMI_OK && (first < numBlocks || first == 0); first += chunk)
            {
                const size_t n = (numBlocks - first) < chunk ? (numBlocks - first) : chunk;
                cvttmi_error_totals part;
                if (n && ((e = hipMemcpyAsync(dBc, bc + first * bcBytes, n * bcBytes, hipMemcpyHostToDevice, stream)) != hipSuccess ||
                          (e = hipMemcpyAsync(dSrc, static_cast<const uint8_t *>(source) + first * texBytes, n * texBytes, hipMemcpyHostToDevice, stream)) != hipSuccess))
                {
                    rc = fail(ctx, CVTTMI_E_HIP, "H2D", e);
                    break;
                }
                if ((rc = timed(ctx, stream, [&] { return measureLaunches(ctx, format, dBc, dSrc, 0, 0, 0, 0, n, dErr, dTot, stream); })) != CVTTMI_OK)
                    break;
                if ((e = hipMemcpyAsync(&part, dTot, sizeof(part), hipMemcpyDeviceToHost, stream)) != hipSuccess ||
                    (dErr && n && (e = hipMemcpyAsync(static_cast<uint8_t *>(blockError) + first * 4, dErr, n * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) ||
                    (e = hipStreamSynchronize(stream)) != hipSuccess)
                {
                    rc = fail(ctx, CVTTMI_E_HIP, "measure", e);
                    break;
                }
                for (int c = 0; c < 4; c++)
                {
                    sum.sse[c] += part.sse[c];
                    sum.sseHdr[c] += part.sseHdr[c];
                }
                sum.texels += part.texels;
            }
            (void)hipStreamSynchronize(stream);
            if (rc == CVTTMI_OK)
                memcpy(totals, &sum, sizeof(sum)); // (host pointers need no alignment)
            return rc;
        });
    }

    int cvttmi_measure_image_error_device(cvttmi_context *ctx, int format, const void *d_bc, const void *d_image, uint32_t width,
                                          uint32_t height, size_t rowPitchBytes, int pixels, void *d_blockError,
                                          cvttmi_error_totals *d_totals, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        size_t bcBytes = 0;
        const size_t bpp = imageTexelBytes(format, pixels, &bcBytes); // 0: not the image kind of the format's row
        const size_t numBlocks = (((size_t)width + 3) / 4) * (((size_t)height + 3) / 4);
        if (bpp == 0 || !d_bc || !d_image || !d_totals || width == 0 || height == 0 || rowPitchBytes < (size_t)width * bpp ||
            (rowPitchBytes % bpp) != 0 || numBlocks > kMaxLaunchBlocks)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (!alignedTo(d_bc, bcBytes) || !alignedTo(d_image, bpp) || !alignedTo(d_blockError, 4) || !alignedTo(d_totals, 8))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        hipStream_t stream = static_cast<hipStream_t>(hipStream);
        return withDevice(ctx, [&] {
            return timed(ctx, stream, [&] {
                return measureLaunches(ctx, format, d_bc, d_image, 1 + pixels, width, height, rowPitchBytes, numBlocks, d_blockError, d_totals, stream);
            });
        });
    }

    // ---- packed blocks -> linear images (cvtt_mi355x.h, "decoding into images"): no context work space, one launch each ----
    int cvttmi_decode_image_device(cvttmi_context *ctx, int format, void *d_image, size_t rowPitchBytes, int pixels, const void *d_bc,
                                   uint32_t width, uint32_t height, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        size_t bcBytes = 0;
        const size_t texel = imageTexelBytes(format, pixels, &bcBytes);
        const size_t numBlocks = (((size_t)width + 3) / 4) * (((size_t)height + 3) / 4);
        if (texel == 0 || !d_image || !d_bc || width == 0 || height == 0 || rowPitchBytes < (size_t)width * texel ||
            (rowPitchBytes % texel) != 0 || numBlocks > kMaxLaunchBlocks)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (!alignedTo(d_bc, bcBytes) || !alignedTo(d_image, texel))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        hipStream_t stream = static_cast<hipStream_t>(hipStream);
        return withDevice(ctx, [&] {
            return timed(ctx, stream, [&] {
                const hipError_t e = cvttmi_launch_decode_image(d_bc, d_image, rowPitchBytes, width, height, format, ctx->tables(), stream);
                return e == hipSuccess ? CVTTMI_OK : fail(ctx, CVTTMI_E_HIP, "decode image kernel launch", e);
            });
        });
    }

    int cvttmi_decode_mips_device(cvttmi_context *ctx, int format, void *d_image, size_t rowPitchBytes, void *d_pyramid, size_t pyramidBytes,
                                  int pixels, const void *d_bc, uint32_t width, uint32_t height, uint32_t levels, void *hipStream)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        size_t bcBytes = 0;
        const size_t texel = imageTexelBytes(format, pixels, &bcBytes);
        if (texel == 0 || !d_image || !d_bc || width == 0 || height == 0 || rowPitchBytes < (size_t)width * texel || (rowPitchBytes % texel) != 0)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        cvttmi_mip_level table[kMaxMipLevels + 1];
        if (cvttmi_mip_layout(width, height, pixels, static_cast<uint32_t>(bcBytes), levels, table) != CVTTMI_OK || (levels > 1 && !d_pyramid) ||
            table[levels].firstBlock > kMaxLaunchBlocks)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (pyramidBytes < table[levels].byteOffset)
            return fail(ctx, CVTTMI_E_INVALID, "pyramid buffer smaller than cvttmi_mip_layout asks for");
        if (!alignedTo(d_bc, bcBytes) || !alignedTo(d_image, texel) || !alignedTo(d_pyramid, texel))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        static_assert(kCvttDecodeLevels >= kMaxMipLevels, "the level table of the mips kernel");
        CvttDecodeLevels args;
        memset(&args, 0, sizeof(args));
        for (uint32_t l = 0; l < levels; l++)
        {
            CvttDecodeLevel &L = args.level[l];
            L.image = l == 0 ? static_cast<uint8_t *>(d_image) : static_cast<uint8_t *>(d_pyramid) + table[l].byteOffset;
            L.pitch = l == 0 ? rowPitchBytes : table[l].rowPitchBytes;
            L.width = table[l].width;
            L.height = table[l].height;
            L.firstBlock = static_cast<uint32_t>(table[l].firstBlock);
            L.blocksPerRow = static_cast<uint32_t>(((uint64_t)table[l].width + 3) / 4);
        }
        args.count = levels;
        args.numBlocks = static_cast<uint32_t>(table[levels].firstBlock);
        hipStream_t stream = static_cast<hipStream_t>(hipStream);
        return withDevice(ctx, [&] {
            return timed(ctx, stream, [&] {
                const hipError_t e = cvttmi_launch_decode_mips(d_bc, &args, format, ctx->tables(), stream);
                return e == hipSuccess ? CVTTMI_OK : fail(ctx, CVTTMI_E_HIP, "decode mips kernel launch", e);
            });
        });
    }

    double cvttmi_psnr(const cvttmi_error_totals *t, uint32_t channelMask)
    {
        uint32_t fmask = 0;
        const CvttTextureFormat *row = t ? formatInfo(t->format, NULL, NULL, &fmask) : NULL;
        if (!row || row->peak == 0) // (BC6H: no PSNR)
            return NAN;
        const uint32_t m = channelMask ? channelMask : fmask;
        if ((m & ~fmask) != 0 || t->texels == 0)
            return NAN;
        uint64_t sse = 0;
        int channels = 0;
        for (int c = 0; c < 4; c++)
            if ((m >> c) & 1u)
            {
                sse += t->sse[c];
                channels++;
            }
        if (sse == 0)
            return INFINITY;
        const double peak = row->peak;
        const double mse = static_cast<double>(sse) / (static_cast<double>(t->texels) * channels);
        return 10.0 * log10(peak * peak / mse);
    }
}
