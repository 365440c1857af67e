// Lane-test kernels over cvtt_kernel_common.h and bc6h_quant.h: every function is the product header's own, compiled with
// the product's device flags; this file only feeds them their domains and stores or compares what they return.
#include "cvtt_kernel_common.h"
#include <hip/hip_fp16.h>
#include "bc6h_quant.h"
#include "lanetest_device.h"

// ---- float lane operations on all 2^32 patterns (the host compares with the SSE2 sequence) ----
LANETEST_SWEEP32(clamp_round, (int)clampRound(v, hi))
LANETEST_SWEEP32(clamp_high_byte, __builtin_amdgcn_cvt_pk_u8_f32(clampHigh(v, hi), 0u, 0u))
LANETEST_SWEEP32(round_clamp_low, __float_as_uint(roundClampLow(clampHigh(v, hi))))
LANETEST_SWEEP32(endpoint_byte, endpointByte(v))
LANETEST_SWEEP32(safe_denom, __float_as_uint(safeDenom(v)))

namespace
{
__global__ void pairOpsKernel(const float *__restrict__ a, const float *__restrict__ b, u32 n, float *__restrict__ outMin,
                              float *__restrict__ outMax)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    outMin[i] = sseMin(a[i], b[i]);
    outMax[i] = sseMax(a[i], b[i]);
}

__global__ void halfToFloatKernel(u32 *__restrict__ outUnsigned, u32 *__restrict__ outSigned)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; // 65 536 threads
    outUnsigned[i] = __float_as_uint(twosCLHalfToFloat<false>((int)i));
    outSigned[i] = __float_as_uint(twosCLHalfToFloat<true>((int)i));
}

__global__ void ceilDiv31Kernel(u32 n, int *__restrict__ out)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = ceilDiv31((int)i);
}

__global__ void quantizeKernel(const int *__restrict__ elem, const int *__restrict__ prec, u32 n, int isSigned, int *__restrict__ out)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = isSigned ? quantizeSigned(elem[i], prec[i]) : quantizeUnsigned(elem[i], prec[i]);
}

__global__ void unquantizeKernel(const int *__restrict__ comp, const int *__restrict__ prec, u32 n, int isSigned, int *__restrict__ outUnq,
                                 int *__restrict__ outFinished)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    int fin = 0;
    outUnq[i] = isSigned ? unquantizeSigned(comp[i], prec[i], fin) : unquantizeUnsigned(comp[i], prec[i], fin);
    outFinished[i] = fin;
}

__global__ void mulU24Kernel(const u32 *__restrict__ a, const u32 *__restrict__ b, u32 n, u32 *__restrict__ out)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = mulU24(a[i], b[i]);
}

// deltaOf(v, base, lost) and deltaFits of the mode word that holds `lost` for channel i % 3
__global__ void deltaKernel(const int *__restrict__ v, const int *__restrict__ base, const int *__restrict__ lost, const int *__restrict__ mask, u32 n,
                            int *__restrict__ outDelta, int *__restrict__ outFits)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const int ch = (int)(i % 3u);
    const u32 mw = 16u | ((u32)lost[i] << (8 + 8 * ch));
    outDelta[i] = deltaOf(v[i], base[i], lostBitsOf(mw, ch));
    outFits[i] = deltaFits(mw, v[i], base[i], ch, mask[i]) ? 1 : 0;
}

__global__ void tweakOfKernel(int *__restrict__ out)
{
    out[threadIdx.x] = tweakOf((int)threadIdx.x); // 12 threads
}

// ---- the 24-bit interpolant of BC6H against the two full multiplications ----
// variant: 0 / 1 reconstructFrom<false, true / false>, 2 / 3 reconstructFrom<true, true / false>, 4 / 5 reconstructChannel<false / true>
template <int VARIANT>
__device__ __forceinline__ int reconstructUnderTest(int e0, int e1, int w)
{
    if (VARIANT == 0) return reconstructFrom<false, true>(e0 * 64 + 32, e1 - e0, w);
    if (VARIANT == 1) return reconstructFrom<false, false>(e0 * 64 + 32, e1 - e0, w);
    if (VARIANT == 2) return reconstructFrom<true, true>(e0 * 64 + 32, e1 - e0, w);
    if (VARIANT == 3) return reconstructFrom<true, false>(e0 * 64 + 32, e1 - e0, w);
    if (VARIANT == 4) return reconstructChannel<false>(e0, e1, w);
    return reconstructChannel<true>(e0, e1, w);
}

// (64 - w) e0 + w e1 with two 32-bit multiplications, + 32, >> 6, the conversion to 16 bits, then the unscaling
template <bool SIGNED>
__device__ __forceinline__ int reconstructPlain(int e0, int e1, int w)
{
    const int p32 = ((64 - w) * e0 + w * e1 + 32) >> 6;
    if (SIGNED)
    {
        const int p = p32 > 32767 ? 32767 : (p32 < -32768 ? -32768 : p32);
        const int a = p < 0 ? -p : p;
        int scaled = (a * 31) >> 5;
        scaled = scaled > 32767 ? 32767 : scaled;
        return (int)(short)(unsigned short)(scaled | (p < 0 ? 0x8000 : 0));
    }
    return (int)((((u32)p32 & 0xffffu) * 31u) >> 6);
}

// one thread per e0 (65 536), all weights x all e1 of the list.  An input's number: e0 index << 32 | e1 index << 8 | weight index
template <int VARIANT>
__global__ void reconstructKernel(const int *__restrict__ e1List, u32 n1, const int *__restrict__ weights, u32 nw, unsigned long long *__restrict__ result)
{
    constexpr bool SIGNED = VARIANT == 2 || VARIANT == 3 || VARIANT == 5;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e0 = SIGNED ? (int)t - 32768 : (int)t;
    unsigned long long mine = 0, first = ~0ull;
    for (u32 i = 0; i < n1; i++)
        for (u32 k = 0; k < nw; k++)
        {
            const int e1 = e1List[i], w = weights[k];
            if (reconstructUnderTest<VARIANT>(e0, e1, w) != reconstructPlain<SIGNED>(e0, e1, w))
            {
                const unsigned long long id = ((unsigned long long)t << 32) | ((unsigned long long)i << 8) | k;
                mine++;
                first = first < id ? first : id;
            }
        }
    lanetestReport(result, mine, first);
}

// ---- the reconstruct-and-compare step of the BC7 chain (bc7_chain.h: recBase = ((e0 << 6) + 32) << 2, recDelta = (e1 - e0) << 2,
// the weight 0 ... 64) against ((64 - w) e0 + w e1 + 32) >> 6 minus the pixel's byte, squared, plus the running sum ----
// one thread per (e0, e1), every weight x every pixel byte; the pixel's other three bytes hold other values.  An input's
// number: e0 << 24 | e1 << 16 | w << 8 | pixel byte
template <int CH>
__global__ void channelErrorKernel(unsigned long long *__restrict__ result)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e0 = (int)(t >> 8), e1 = (int)(t & 255u);
    const int base4 = ((e0 << 6) + 32) << 2, delta4 = (e1 - e0) << 2;
    unsigned long long mine = 0, first = ~0ull;
    for (int w = 0; w <= 64; w++)
    {
        const int rec = ((64 - w) * e0 + w * e1 + 32) >> 6;
        const int sum = madI24(w, delta4, base4);
        bool bad = sum != w * delta4 + base4;
        for (u32 p = 0; p < 256u; p++)
        {
            const u32 others = (p * 0x9Du + 0x35u) & 255u;
            const u32 pk = ((others | ((others ^ 0xffu) << 8) | ((others ^ 0x5au) << 16) | ((p ^ 0x80u) << 24)) & ~(255u << (8 * CH))) | (p << (8 * CH));
            const int d = rec - (int)p;
            const u32 acc = (u32)(t * 2654435761u) >> 4;
            bool wrong = bad;
            wrong |= subByte1<CH>(sum, pk) != d;
            wrong |= channelError<CH>(w, delta4, base4, pk) != (u32)(d * d);
            wrong |= accumulateChannelError<CH>(w, delta4, base4, pk, acc) != (u32)(d * d) + acc;
            if (wrong)
            {
                const unsigned long long id = ((unsigned long long)t << 16) | ((unsigned long long)w << 8) | p;
                mine++;
                first = first < id ? first : id;
            }
        }
    }
    lanetestReport(result, mine, first);
}

// subByteK<K, CH>(recs, pk) = byte K of recs - byte CH of pk, every pair of bytes, the other bytes of both words set to other
// values.  One thread per pair; an input's number: instance (4 K + CH) << 16 | byte of recs << 8 | byte of pk
template <int K, int CH>
__device__ __forceinline__ bool subByteKWrong(u32 x, u32 y)
{
    const u32 fill = (x * 0x3Bu + y * 0x71u + 0x1Du) & 255u;
    const u32 recs = ((fill * 0x01010101u) & ~(255u << (8 * K))) | (x << (8 * K));
    const u32 pk = (((fill ^ 0xA5u) * 0x01010101u) & ~(255u << (8 * CH))) | (y << (8 * CH));
    return subByteK<K, CH>(recs, pk) != (int)x - (int)y;
}
template <int K>
__device__ __forceinline__ u32 subByteKWrongMask(u32 x, u32 y)
{
    return (subByteKWrong<K, 0>(x, y) ? 1u : 0u) | (subByteKWrong<K, 1>(x, y) ? 2u : 0u) | (subByteKWrong<K, 2>(x, y) ? 4u : 0u) |
           (subByteKWrong<K, 3>(x, y) ? 8u : 0u);
}
__global__ void subByteKKernel(unsigned long long *__restrict__ result)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x; // 65 536 threads
    const u32 x = t >> 8, y = t & 255u;
    const u32 wrong = subByteKWrongMask<0>(x, y) | (subByteKWrongMask<1>(x, y) << 4) | (subByteKWrongMask<2>(x, y) << 8);
    unsigned long long mine = 0, first = ~0ull;
    for (u32 inst = 0; inst < 12u; inst++)
        if ((wrong >> inst) & 1u)
        {
            const unsigned long long id = ((unsigned long long)inst << 16) | t;
            mine++;
            first = first < id ? first : id;
        }
    lanetestReport(result, mine, first);
}

inline dim3 blocksFor(u32 n) { return dim3((n + 255u) / 256u); }
} // namespace

extern "C" hipError_t lanetest_pair_ops(const void *d_a, const void *d_b, uint32_t n, void *d_min, void *d_max, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(pairOpsKernel, blocksFor(n), dim3(256), 0, stream, (const float *)d_a, (const float *)d_b, n, (float *)d_min, (float *)d_max);
    return hipGetLastError();
}

// both outputs: 65 536 words
extern "C" hipError_t lanetest_half_to_float(void *d_unsigned, void *d_signed, hipStream_t stream)
{
    hipLaunchKernelGGL(halfToFloatKernel, dim3(256), dim3(256), 0, stream, (u32 *)d_unsigned, (u32 *)d_signed);
    return hipGetLastError();
}

extern "C" hipError_t lanetest_ceil_div31(uint32_t n, void *d_out, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(ceilDiv31Kernel, blocksFor(n), dim3(256), 0, stream, n, (int *)d_out);
    return hipGetLastError();
}

extern "C" hipError_t lanetest_quantize(const void *d_elem, const void *d_prec, uint32_t n, int isSigned, void *d_out, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(quantizeKernel, blocksFor(n), dim3(256), 0, stream, (const int *)d_elem, (const int *)d_prec, n, isSigned, (int *)d_out);
    return hipGetLastError();
}

extern "C" hipError_t lanetest_unquantize(const void *d_comp, const void *d_prec, uint32_t n, int isSigned, void *d_unq, void *d_finished,
                                          hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(unquantizeKernel, blocksFor(n), dim3(256), 0, stream, (const int *)d_comp, (const int *)d_prec, n, isSigned, (int *)d_unq,
                       (int *)d_finished);
    return hipGetLastError();
}

extern "C" hipError_t lanetest_mul_u24(const void *d_a, const void *d_b, uint32_t n, void *d_out, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(mulU24Kernel, blocksFor(n), dim3(256), 0, stream, (const u32 *)d_a, (const u32 *)d_b, n, (u32 *)d_out);
    return hipGetLastError();
}

extern "C" hipError_t lanetest_delta(const void *d_v, const void *d_base, const void *d_lost, const void *d_mask, uint32_t n, void *d_delta,
                                     void *d_fits, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(deltaKernel, blocksFor(n), dim3(256), 0, stream, (const int *)d_v, (const int *)d_base, (const int *)d_lost,
                       (const int *)d_mask, n, (int *)d_delta, (int *)d_fits);
    return hipGetLastError();
}

// d_out: 12 words
extern "C" hipError_t lanetest_tweak_of(void *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(tweakOfKernel, dim3(1), dim3(12), 0, stream, (int *)d_out);
    return hipGetLastError();
}

// d_result: two 64-bit words, {0, ~0} on entry (lanetest_device.h), here and below
extern "C" hipError_t lanetest_reconstruct(int variant, const void *d_e1, uint32_t n1, const void *d_weights, uint32_t nw, void *d_result,
                                           hipStream_t stream)
{
    const int *e1 = (const int *)d_e1, *w = (const int *)d_weights;
    unsigned long long *r = (unsigned long long *)d_result;
    switch (variant)
    {
    case 0: hipLaunchKernelGGL(reconstructKernel<0>, dim3(256), dim3(256), 0, stream, e1, n1, w, nw, r); break;
    case 1: hipLaunchKernelGGL(reconstructKernel<1>, dim3(256), dim3(256), 0, stream, e1, n1, w, nw, r); break;
    case 2: hipLaunchKernelGGL(reconstructKernel<2>, dim3(256), dim3(256), 0, stream, e1, n1, w, nw, r); break;
    case 3: hipLaunchKernelGGL(reconstructKernel<3>, dim3(256), dim3(256), 0, stream, e1, n1, w, nw, r); break;
    case 4: hipLaunchKernelGGL(reconstructKernel<4>, dim3(256), dim3(256), 0, stream, e1, n1, w, nw, r); break;
    case 5: hipLaunchKernelGGL(reconstructKernel<5>, dim3(256), dim3(256), 0, stream, e1, n1, w, nw, r); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" hipError_t lanetest_channel_error(int channel, void *d_result, hipStream_t stream)
{
    unsigned long long *r = (unsigned long long *)d_result;
    switch (channel)
    {
    case 0: hipLaunchKernelGGL(channelErrorKernel<0>, dim3(256), dim3(256), 0, stream, r); break;
    case 1: hipLaunchKernelGGL(channelErrorKernel<1>, dim3(256), dim3(256), 0, stream, r); break;
    case 2: hipLaunchKernelGGL(channelErrorKernel<2>, dim3(256), dim3(256), 0, stream, r); break;
    case 3: hipLaunchKernelGGL(channelErrorKernel<3>, dim3(256), dim3(256), 0, stream, r); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" hipError_t lanetest_sub_byte_k(void *d_result, hipStream_t stream)
{
    hipLaunchKernelGGL(subByteKKernel, dim3(256), dim3(256), 0, stream, (unsigned long long *)d_result);
    return hipGetLastError();
}
