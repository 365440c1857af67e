// Lane-test kernels over etc2_metric.h: the fake-BT.709 resolvers, the three metrics, planarDecode and the T / H emitters are
// the product header's own, compiled with the product's device flags; this file feeds them the domains of
// oracle/etc_parts.h (shared with the host references, which walk the same input numbers) and stores what they return, or
// decodes an emitted block with the product's own decoder (decode_texels.h) and compares the texels.
#include <string.h>
#include "cvtt_kernel_common.h"
#include "cvtt_device.h"
#include "etc2_wave.h"
#include "etc2_metric.h"
#include "decode_texels.h"
#include "etc_tables.h"
#include "fake709_rounding.h"
#include "lanetest_device.h"
#include "../../oracle/etc_parts.h"

namespace
{
struct EtcSweep
{
    int part, variant;
    float rw, gw, bw;
    const int32_t *table;                // the sweep's own table (etc_parts.h), device memory
    const CvttDeviceTables *tables;      // thDistance, etc1Modifiers, fake709Rounding filled (lanetest_etc_tables)
};

__device__ __forceinline__ uint32_t evalPart(const EtcSweep &s, uint32_t n)
{
    switch (s.part)
    {
    case ETCP_RESOLVE_TH:
    {
        int g, targets[3], q[3];
        etcp_th_args(s.table, n, &g, targets, q);
        resolveTHFake(q, targets, g);
        return etcp_pack3(q, 15);
    }
    case ETCP_RESOLVE_HALF:
    {
        int cumulative[3], q[3] = {0, 0, 0};
        etcp_half_args(s.table, n, cumulative);
        resolveHalfFake(q, cumulative, (s.variant & 1) != 0, (s.variant & 2) != 0, s.tables);
        return etcp_pack3(q, etcp_half_limit(s.variant));
    }
    case ETCP_ERR_FAKE:
    case ETCP_ERR_WU:
    case ETCP_ERR2:
    {
        int rec[3], px[3];
        float pw[3];
        etcp_err_args(s.table, n, rec, px, pw);
        EtcErr E;
        E.uniform = s.part == ETCP_ERR_WU && s.variant == 0;
        E.rw = s.rw;
        E.gw = s.gw;
        E.bw = s.bw;
        E.fake = s.part == ETCP_ERR_FAKE;
        if (s.part == ETCP_ERR_FAKE)
            return etcp_float_bits(E(rec[0], rec[1], rec[2], px, pw));
        if (s.part == ETCP_ERR_WU)
            return etcp_float_bits(E.wu(rec[0], rec[1], rec[2], px, pw));
        int other[3];
        etcp_err2_partner(n, other);
        v2f mw[3];
        E.weigh2(mw, rec, other);
        const v2f e = E.err2(mw, pw);
        return etcp_float_bits(s.variant == 1 ? e.y : e.x);
    }
    case ETCP_PLANAR:
        return (uint32_t)planarDecode((int)(n & 127u), (int)((n >> 7) & 3u));
    case ETCP_EMIT_T:
    {
        etcp_t_args a;
        etcp_t_args_of(n, s.variant & 2, etcp_pattern_of(n), &a);
        u32 hi, lo;
        emitT(hi, lo, a.line, a.iso, a.selectors, a.table, a.opaque != 0);
        return (s.variant & 1) ? lo : hi;
    }
    case ETCP_EMIT_H:
    {
        etcp_h_args a;
        etcp_h_args_of(n, s.variant & 2, etcp_pattern_of(n), &a);
        u32 hi, lo;
        emitH(hi, lo, a.bc[0], a.bc[1], a.sector, a.sign, a.table, a.opaque != 0);
        return (s.variant & 1) ? lo : hi;
    }
    }
    return 0;
}

// sums[t] = the checksum of chunk firstChunk + t
__global__ void etcSumsKernel(EtcSweep s, uint32_t firstChunk, uint32_t numChunks, uint64_t *__restrict__ sums)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numChunks)
        return;
    const uint32_t base = (firstChunk + t) * ETCP_CHUNK;
    uint64_t acc = 0;
    for (uint32_t j = 0; j < ETCP_CHUNK; j++)
        acc += lanetest::term(evalPart(s, base + j), j);
    sums[t] = acc;
}

// out[j] = the result of input chunk * 4096 + j: 16 workgroups of 256 lanes
__global__ void etcChunkKernel(EtcSweep s, uint32_t chunk, uint32_t *__restrict__ out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    out[j] = evalPart(s, chunk * ETCP_CHUNK + j);
}

// ---- the emitted block through the product's decoder --------------------------------------------------------------------
// What the block must decode to is stated from the emitter's ARGUMENTS and the format (the mode a decoder takes from the
// overflow of the differential sums; index 2 of a block without the opaque bit is transparent), never from the emitter.
__device__ __forceinline__ int signed3(int d) { return d >= 4 ? d - 8 : d; }

// 1: T, 2: H, 3: planar, 0: individual / differential -- the format's rule on the block's bits
__device__ __forceinline__ int modeOfBits(u64 w)
{
    const int r2 = bitsOf(w, 59, 5) + signed3(bitsOf(w, 56, 3)), g2 = bitsOf(w, 51, 5) + signed3(bitsOf(w, 48, 3));
    const int b2 = bitsOf(w, 43, 5) + signed3(bitsOf(w, 40, 3));
    return (r2 < 0 || r2 > 31) ? 1 : (g2 < 0 || g2 > 31) ? 2 : (b2 < 0 || b2 > 31) ? 3 : 0;
}

__device__ __forceinline__ void decodeEmitted(u32 hi, u32 lo, bool opaque, const CvttDeviceTables *T, int px[16][4])
{
    const u64 w = ((u64)hi << 32) | lo;
    if (opaque)
        etcColour<false>(w, T, px);
    else
        etcColour<true>(w, T, px);
}

// texel p must be `colour` + delta on every channel, clamped, opaque; or transparent black
__device__ __forceinline__ bool texelWrong(const int got[4], const int colour[3], int delta, bool transparent)
{
    bool wrong = false;
#pragma unroll
    for (int c = 0; c < 3; c++)
        wrong |= got[c] != (transparent ? 0 : clamp255(colour[c] * 17 + delta));
    return wrong | (got[3] != (transparent ? 0 : 255));
}

__device__ __forceinline__ bool tRoundTripWrong(const etcp_t_args &a, const CvttDeviceTables *T)
{
    u32 hi, lo;
    emitT(hi, lo, a.line, a.iso, a.selectors, a.table, a.opaque != 0);
    if (modeOfBits(((u64)hi << 32) | lo) != 1 || (((hi >> 1) & 1u) != 0) != (a.opaque != 0))
        return true;
    int px[16][4];
    decodeEmitted(hi, lo, a.opaque != 0, T, px);
    const int d = T->thDistance[a.table];
    bool wrong = false;
#pragma unroll
    for (int p = 0; p < 16; p++)
    {
        const int sel = (int)((a.selectors >> (2 * p)) & 3u);
        wrong |= texelWrong(px[p], sel == 0 ? a.iso : a.line, sel == 1 ? d : sel == 3 ? -d : 0, !a.opaque && sel == 2);
    }
    return wrong;
}

__device__ __forceinline__ bool hRoundTripWrong(const etcp_h_args &a, const CvttDeviceTables *T)
{
    const bool equal = a.bc[0] == a.bc[1];
    if (equal && !a.opaque)
        return false; // index 2 cannot be avoided there: only the reference's bytes hold (the comparison with its emitter)
    u32 hi, lo;
    emitH(hi, lo, a.bc[0], a.bc[1], a.sector, a.sign, a.table, a.opaque != 0);
    if (modeOfBits(((u64)hi << 32) | lo) != (equal ? 1 : 2) || (((hi >> 1) & 1u) != 0) != (a.opaque != 0))
        return true;
    int px[16][4];
    decodeEmitted(hi, lo, a.opaque != 0, T, px);
    const int d = T->thDistance[a.table];
    int colours[2][3];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            colours[s][c] = (a.bc[s] >> (5 * (2 - c))) & 15;
    bool wrong = false;
#pragma unroll
    for (int p = 0; p < 16; p++)
    {
        const int x = p & 3, y = p >> 2, slot = 4 * x + y;
        const int formatIndex = (int)((((lo >> (16 + slot)) & 1u) << 1) | ((lo >> slot) & 1u));
        const bool second = ((a.sector >> p) & 1u) != 0, minus = ((a.sign >> p) & 1u) != 0;
        wrong |= texelWrong(px[p], second ? colours[1] : colours[0], minus ? -d : d, !a.opaque && formatIndex == 2);
    }
    return wrong;
}

// every input of the emitter's full domain (2^28) x the four patterns; one thread per 4096 inputs.  An input's number:
// n << 2 | pattern
template <bool H>
__global__ void roundTripKernel(const CvttDeviceTables *__restrict__ T, unsigned long long *__restrict__ result)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; // 65 536 threads
    unsigned long long mine = 0, first = ~0ull;
    for (uint32_t j = 0; j < ETCP_CHUNK; j++)
    {
        const uint32_t n = t * ETCP_CHUNK + j;
        for (int pattern = 0; pattern < 4; pattern++)
        {
            bool wrong;
            if (H)
            {
                etcp_h_args a;
                etcp_h_args_of(n, 0, pattern, &a);
                wrong = hRoundTripWrong(a, T);
            }
            else
            {
                etcp_t_args a;
                etcp_t_args_of(n, 0, pattern, &a);
                wrong = tRoundTripWrong(a, T);
            }
            if (wrong)
            {
                const unsigned long long id = ((unsigned long long)n << 2) | (unsigned long long)pattern;
                mine++;
                first = first < id ? first : id;
            }
        }
    }
    lanetestReport(result, mine, first);
}

// the blocks of listed inputs in the format's byte order, and their texels as the in-kernel decoder gives them (RGBA bytes)
__global__ void emitSampleKernel(int part, const uint32_t *__restrict__ inputs, uint32_t count, const CvttDeviceTables *__restrict__ T,
                                 uint8_t *__restrict__ blocks, uint8_t *__restrict__ texels)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t n = inputs[i];
    u32 hi, lo;
    bool opaque;
    if (part == ETCP_EMIT_H)
    {
        etcp_h_args a;
        etcp_h_args_of(n, 0, etcp_pattern_of(n), &a);
        emitH(hi, lo, a.bc[0], a.bc[1], a.sector, a.sign, a.table, a.opaque != 0);
        opaque = a.opaque != 0;
    }
    else
    {
        etcp_t_args a;
        etcp_t_args_of(n, 0, etcp_pattern_of(n), &a);
        emitT(hi, lo, a.line, a.iso, a.selectors, a.table, a.opaque != 0);
        opaque = a.opaque != 0;
    }
    for (int b = 0; b < 4; b++)
    {
        blocks[i * 8u + b] = (uint8_t)(hi >> (24 - 8 * b));
        blocks[i * 8u + 4 + b] = (uint8_t)(lo >> (24 - 8 * b));
    }
    int px[16][4];
    decodeEmitted(hi, lo, opaque, T, px);
    for (int p = 0; p < 16; p++)
        for (int c = 0; c < 4; c++)
            texels[i * 64u + p * 4 + c] = (uint8_t)px[p][c];
}

EtcSweep makeSweep(int part, int variant, const float *weights3, const void *d_table, const void *d_tables)
{
    EtcSweep s;
    s.part = part;
    s.variant = variant;
    s.rw = weights3 ? weights3[0] : 0.0f;
    s.gw = weights3 ? weights3[1] : 0.0f;
    s.bw = weights3 ? weights3[2] : 0.0f;
    s.table = (const int32_t *)d_table;
    s.tables = (const CvttDeviceTables *)d_tables;
    return s;
}
} // namespace

extern "C" size_t lanetest_etc_tables_size(void) { return sizeof(CvttDeviceTables); }

// d_tables: lanetest_etc_tables_size() bytes.  The three members the ETC functions read, from the product's own table headers
// (the rest zero); the copy is made before this returns.
extern "C" hipError_t lanetest_etc_tables(void *d_tables, hipStream_t stream)
{
    static CvttDeviceTables t;
    memset(&t, 0, sizeof(t));
    for (int i = 0; i < 8; i++)
    {
        for (int k = 0; k < 4; k++)
            t.etc1Modifiers[i][k] = k_etc1_modifiers[i * 4 + k];
        t.thDistance[i] = k_th_distance[i];
    }
    memcpy(t.fake709Rounding, k_fake709Rounding16, sizeof(t.fake709Rounding));
    hipError_t rc = hipMemcpyAsync(d_tables, &t, sizeof(t), hipMemcpyHostToDevice, stream);
    return rc != hipSuccess ? rc : hipStreamSynchronize(stream);
}

// weights3: host memory (three floats) or NULL.  d_sums: numChunks 64-bit words
extern "C" hipError_t lanetest_etc_sums(int part, int variant, const float *weights3, const void *d_table, const void *d_tables, uint32_t firstChunk,
                                        uint32_t numChunks, void *d_sums, hipStream_t stream)
{
    if (part < 0 || part >= ETCP_PARTS || (uint64_t)firstChunk + numChunks > etcp_chunks(part, variant))
        return hipErrorInvalidValue;
    if (numChunks == 0)
        return hipSuccess;
    hipLaunchKernelGGL(etcSumsKernel, dim3((numChunks + 255u) / 256u), dim3(256), 0, stream, makeSweep(part, variant, weights3, d_table, d_tables),
                       firstChunk, numChunks, (uint64_t *)d_sums);
    return hipGetLastError();
}

// d_out: 4096 words
extern "C" hipError_t lanetest_etc_chunk(int part, int variant, const float *weights3, const void *d_table, const void *d_tables, uint32_t chunk,
                                         void *d_out, hipStream_t stream)
{
    if (part < 0 || part >= ETCP_PARTS || chunk >= etcp_chunks(part, variant))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(etcChunkKernel, dim3(ETCP_CHUNK / 256u), dim3(256), 0, stream, makeSweep(part, variant, weights3, d_table, d_tables), chunk,
                       (uint32_t *)d_out);
    return hipGetLastError();
}

// d_result: two 64-bit words, {0, ~0} on entry (lanetest_device.h)
extern "C" hipError_t lanetest_etc_round_trip(int part, const void *d_tables, void *d_result, hipStream_t stream)
{
    const CvttDeviceTables *T = (const CvttDeviceTables *)d_tables;
    unsigned long long *r = (unsigned long long *)d_result;
    if (part == ETCP_EMIT_T)
        hipLaunchKernelGGL(roundTripKernel<false>, dim3(256), dim3(256), 0, stream, T, r);
    else if (part == ETCP_EMIT_H)
        hipLaunchKernelGGL(roundTripKernel<true>, dim3(256), dim3(256), 0, stream, T, r);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// d_inputs: count input numbers of the emitter's full domain; d_blocks: 8 bytes each; d_texels: 64 bytes each
extern "C" hipError_t lanetest_etc_emit_sample(int part, const void *d_inputs, uint32_t count, const void *d_tables, void *d_blocks, void *d_texels,
                                               hipStream_t stream)
{
    if (part != ETCP_EMIT_T && part != ETCP_EMIT_H)
        return hipErrorInvalidValue;
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(emitSampleKernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, part, (const uint32_t *)d_inputs, count,
                       (const CvttDeviceTables *)d_tables, (uint8_t *)d_blocks, (uint8_t *)d_texels);
    return hipGetLastError();
}
