// Lane-test kernels over resample_common.h and mip_common.h: the byte a rule's sum or quotient becomes, the sRGB encode through
// both table layouts, and the box rule on four bytes at once.  The functions are the product headers' own, compiled with the
// product's device flags.
#include "resample_common.h"
#include "lanetest_device.h"

// plainByte<KIND>(s) on all 2^32 sums.  (hi is not used.)
LANETEST_SWEEP32(plain_byte_u8, plainByte<kRGBA8>((int)bits))
LANETEST_SWEEP32(plain_byte_s8, plainByte<kRGBA8Snorm>((int)bits))
// normalByte<KIND>(q) for every |q| <= 1 + 2^-20 (0x3f800008); 0 stands for every other pattern, NaNs included
LANETEST_SWEEP32(normal_byte_u8, (bits & 0x7fffffffu) <= 0x3f800008u ? normalByte<kRGBA8>(v) : 0u)
LANETEST_SWEEP32(normal_byte_s8, (bits & 0x7fffffffu) <= 0x3f800008u ? normalByte<kRGBA8Snorm>(v) : 0u)

namespace
{
// srgbEncode(t, S) for S = 0 ... n - 1 through the mip kernels' layout (outFull) and resize's (outSplit); 256 lanes per
// workgroup, as both loaders expect
__global__ void srgbEncodeKernel(uint32_t n, uint32_t *__restrict__ outFull, uint32_t *__restrict__ outSplit)
{
    __shared__ SrgbTables full;
    __shared__ SrgbEncodeTables split;
    loadSrgbTables(full, blockDim.x, threadIdx.x);
    loadEncode(split);
    __syncthreads();
    const uint32_t S = blockIdx.x * blockDim.x + threadIdx.x;
    if (S >= n)
        return;
    outFull[S] = srgbEncode(full, S);
    outSplit[S] = srgbEncode(split, S);
}

__device__ __forceinline__ uint64_t boxMix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The inputs of box4x8: quadruple i < 1296 = 6^4 is the edge set -- byte k of the four words holds the (i + 433 k) mod 1296-th
// quadruple drawn from {0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF}, so every byte position meets every quadruple, each beside other
// neighbours --, the rest are pseudo-random words.
__device__ __forceinline__ void boxInputs(uint64_t seed, uint32_t i, uint32_t (&w)[4])
{
    if (i < 1296u)
    {
        const uint32_t edge[6] = {0x00u, 0x01u, 0x7Fu, 0x80u, 0xFEu, 0xFFu};
        w[0] = w[1] = w[2] = w[3] = 0;
        for (uint32_t k = 0; k < 4u; k++)
        {
            uint32_t q = (i + 433u * k) % 1296u;
            for (int j = 0; j < 4; j++)
            {
                w[j] |= edge[q % 6u] << (8u * k);
                q /= 6u;
            }
        }
        return;
    }
    const uint64_t r0 = boxMix(seed + (uint64_t)i * 0x9E3779B97F4A7C15ull), r1 = boxMix(r0 + 0x632BE59BD9B4E019ull);
    w[0] = (uint32_t)r0;
    w[1] = (uint32_t)(r0 >> 32);
    w[2] = (uint32_t)r1;
    w[3] = (uint32_t)(r1 >> 32);
}

// against the rule a byte at a time: floor((a + b + c + d + 2) / 4) of the bytes, as uint8 or as int8
template <int KIND>
__global__ void box4x8Kernel(uint64_t seed, uint32_t n, unsigned long long *__restrict__ result)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t w[4];
    boxInputs(seed, i, w);
    uint32_t want = 0;
    for (int k = 0; k < 4; k++)
    {
        int sum = 2;
        for (int j = 0; j < 4; j++)
        {
            const uint32_t byte = (w[j] >> (8 * k)) & 255u;
            sum += KIND == kRGBA8Snorm ? (int)(int8_t)byte : (int)byte;
        }
        want |= ((uint32_t)(sum >> 2) & 255u) << (8 * k);
    }
    if (box4x8<KIND>(w[0], w[1], w[2], w[3]) != want)
        lanetestReport(result, 1ull, (unsigned long long)i);
}

// the four words of quadruple i, for a failure message
__global__ void boxInputsKernel(uint64_t seed, uint32_t i, uint32_t *__restrict__ out)
{
    uint32_t w[4];
    boxInputs(seed, i, w);
    for (int j = 0; j < 4; j++)
        out[j] = w[j];
}
} // namespace

// both outputs: n words
extern "C" hipError_t lanetest_srgb_encode(uint32_t n, void *d_full, void *d_split, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(srgbEncodeKernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, (uint32_t *)d_full, (uint32_t *)d_split);
    return hipGetLastError();
}

// kind: CVTTMI_PIXELS_RGBA8 or CVTTMI_PIXELS_RGBA8_SNORM.  d_result: two 64-bit words, {0, ~0} on entry (lanetest_device.h)
extern "C" hipError_t lanetest_box4x8(int kind, uint64_t seed, uint32_t n, void *d_result, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    unsigned long long *r = (unsigned long long *)d_result;
    if (kind == kRGBA8)
        hipLaunchKernelGGL(box4x8Kernel<kRGBA8>, dim3((n + 255u) / 256u), dim3(256), 0, stream, seed, n, r);
    else if (kind == kRGBA8Snorm)
        hipLaunchKernelGGL(box4x8Kernel<kRGBA8Snorm>, dim3((n + 255u) / 256u), dim3(256), 0, stream, seed, n, r);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// d_out: four words
extern "C" hipError_t lanetest_box4x8_inputs(uint64_t seed, uint32_t i, void *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(boxInputsKernel, dim3(1), dim3(1), 0, stream, seed, i, (uint32_t *)d_out);
    return hipGetLastError();
}
