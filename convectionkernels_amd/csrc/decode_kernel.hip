// Decoding and measuring every format (include/cvtt_mi355x.h, CVTTMI_FMT_*): what is about lanes and memory.  One lane takes
// one packed block, decodes it in registers (decode_texels.h) and either stores the texels -- as a decoded block, or into a
// linear image or mip chain -- or adds up their squared error against a source without writing texels to HBM; they let
// quality be checked on the device (decode + PSNR) independently of bit-exactness.  Every kernel is a template over the format
// id and reads the format's facts from its row (texture_formats.h); forFormat is the one place a runtime id becomes one.
#include "cvtt_kernel_common.h"
#include <hip/hip_fp16.h>
#include <type_traits>
#include <utility>
#include "decode_texels.h"
#include "cvtt_launchers.h"

namespace
{
// ---- packed blocks -> decoded blocks (cvttmi_decode_device).  The store goes by the row's decoded size: 32 B of R11 as int16,
// 64 B of 8-bit texels (PixelBlockU8 / S8), 128 B of BC6H (PixelBlockF16: R | G << 16, B | 0x3C00 << 16 per texel). ----
constexpr u32 kDecodeWG = 256;

template <int F>
__global__ __launch_bounds__(256) void cvttmi_decode_kernel(const uint8_t *__restrict__ bc, uint8_t *__restrict__ out, u32 numBlocks,
                                                          const CvttDeviceTables *__restrict__ T)
{
    const u32 block = blockIdx.x * blockDim.x + threadIdx.x;
    if (block >= numBlocks)
        return;
    int px[16][4];
    decodeTexels<F>(loadPacked<F>(bc, block), T, px);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)block * Fmt<F>::texBytes);
    if (Fmt<F>::texBytes == 32u)
    {
        u32 h[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            h[i] = ((u32)px[2 * i][0] & 0xffffu) | (((u32)px[2 * i + 1][0] & 0xffffu) << 16);
        dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
        dst[1] = make_uint4(h[4], h[5], h[6], h[7]);
    }
    else if (Fmt<F>::texBytes == 64u)
    {
        u32 q[16];
#pragma unroll
        for (int p = 0; p < 16; p++)
            q[p] = ((u32)px[p][0] & 0xffu) | (((u32)px[p][1] & 0xffu) << 8) | (((u32)px[p][2] & 0xffu) << 16) | (((u32)px[p][3] & 0xffu) << 24);
#pragma unroll
        for (int i = 0; i < 4; i++)
            dst[i] = make_uint4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
    }
    else
    {
        u32 w[16][2];
#pragma unroll
        for (int p = 0; p < 16; p++)
        {
            w[p][0] = ((u32)px[p][0] & 0xffffu) | (((u32)px[p][1] & 0xffffu) << 16);
            w[p][1] = ((u32)px[p][2] & 0xffffu) | (((u32)px[p][3] & 0xffffu) << 16);
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
            dst[i] = make_uint4(w[2 * i][0], w[2 * i][1], w[2 * i + 1][0], w[2 * i + 1][1]);
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
                    if (F == CVTTMI_FMT_R11U)
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

// The one dispatch over formats: call(F) with the runtime `format` as a compile-time constant, F() of type int -- every id
// 0 .. CVTTMI_FMT_COUNT - 1, so there is no list of ids to keep.  An unknown id is hipErrorInvalidValue.
template <class Call, int... Fs>
hipError_t forFormat(int format, Call call, std::integer_sequence<int, Fs...>)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((format == Fs && ((e = call(std::integral_constant<int, Fs>())), true)) || ...);
    return e;
}
template <class Call>
hipError_t forFormat(int format, Call call) { return forFormat(format, call, std::make_integer_sequence<int, CVTTMI_FMT_COUNT>()); }

template <int F>
hipError_t launchDecode(const void *d_bc, void *d_out, u32 numBlocks, const CvttDeviceTables *T, hipStream_t stream)
{
    hipLaunchKernelGGL(cvttmi_decode_kernel<F>, dim3((numBlocks + kDecodeWG - 1u) / kDecodeWG), dim3(kDecodeWG), 0, stream, (const uint8_t *)d_bc,
                       (uint8_t *)d_out, numBlocks, T);
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

} // namespace

// packed blocks -> the decoded layout of `format`
extern "C" hipError_t cvttmi_launch_decode(const void *d_bc, void *d_out, uint32_t numBlocks, int format, const CvttDeviceTables *d_tables,
                                           hipStream_t stream)
{
    if (numBlocks == 0)
        return hipSuccess;
    return forFormat(format, [&](auto F) { return launchDecode<F()>(d_bc, d_out, numBlocks, d_tables, stream); });
}

// One launch of the measure (numBlocks <= 2^24, > 0) and its total: source 0 = blocks, 1 + CVTTMI_PIXELS_* = an image of the
// format's kind, so 1 = RGBA8, 2 = RGBA16F (the shim rejects other pairs; image: width, height, pitch, blocks per row =
// ceil(width / 4); d_bc starts at block firstBlock of the image).  d_slab: (2^24 / 256) x 4 x 8 bytes.
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
    return forFormat(format, [&](auto F) {
        constexpr int f = decltype(F)::value;
        auto from = [&](auto SRC) {
            return launchMeasureFormat<f, decltype(SRC)::value>(d_bc, d_source, img, numBlocks, d_blockError, d_slab, d_totals, accumulate, texels, d_tables, stream);
        };
        if (source == 0)
            return from(std::integral_constant<int, 0>());
        if constexpr (Fmt<f>::image)
            if (source == 1 + Fmt<f>::row.image)
                return from(std::integral_constant<int, 1 + Fmt<f>::row.image>());
        return hipErrorInvalidValue;
    });
}

// Packed blocks -> linear images: every format with an image form (the shim rejects R11, and the wrong texel size for a
// format, before it comes here).  d_bc: the ceil(width / 4) x ceil(height / 4) blocks, row-major (fewer than 2^32); d_image:
// width x height texels of 4 bytes (BC6H: 8), `pitch` bytes between rows
extern "C" hipError_t cvttmi_launch_decode_image(const void *d_bc, void *d_image, size_t pitch, uint32_t width, uint32_t height, int format,
                                                 const CvttDeviceTables *d_tables, hipStream_t stream)
{
    DecodeTarget img;
    img.image = (uint8_t *)d_image;
    img.pitch = pitch;
    img.width = width;
    img.height = height;
    return forFormat(format, [&](auto F) {
        if constexpr (Fmt<F()>::image)
            return launchDecodeImage<F()>(d_bc, img, d_tables, stream);
        return hipErrorInvalidValue;
    });
}

// levels->level[0 .. count - 1] in level order, their blocks consecutive in d_bc; 0 < numBlocks < 2^32
extern "C" hipError_t cvttmi_launch_decode_mips(const void *d_bc, const CvttDecodeLevels *levels, int format, const CvttDeviceTables *d_tables,
                                                hipStream_t stream)
{
    if (levels->count == 0 || levels->count > kCvttDecodeLevels || levels->numBlocks == 0)
        return hipErrorInvalidValue;
    return forFormat(format, [&](auto F) {
        if constexpr (Fmt<F()>::image)
            return launchDecodeMips<F()>(d_bc, *levels, d_tables, stream);
        return hipErrorInvalidValue;
    });
}
