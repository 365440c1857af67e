// Arithmetic self-test: the kernels promise the reference's SSE2 lane arithmetic (SURVEY.md
// App. A): IEEE-754 binary32 divide and square root, correctly rounded, denormals kept.  This
// kernel evaluates both on pseudo-random bit patterns with exactly the expressions the encoders
// use (operator/ and sqrtExact, same compiler flags); the host compares with DIVSS / SQRTSS.
#include "cvtt_kernel_common.h"
#include "mfma_i8.h"
#include "cvtt_launchers.h"

namespace
{
__device__ __forceinline__ u64 mix64(u64 z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void cvttmi_selftest_kernel(u64 seed, u64 first, u32 count, u32 *__restrict__ operands, u32 *__restrict__ results)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const u64 r = mix64(seed + (first + i) * 0x9E3779B97F4A7C15ull);
    u32 a = (u32)r, b = (u32)(r >> 32);
    // keep the operands finite; every other bit pattern (zeros, denormals, both signs) stays in
    if ((a & 0x7f800000u) == 0x7f800000u) a ^= 0x00800000u;
    if ((b & 0x7f800000u) == 0x7f800000u) b ^= 0x00800000u;
    const float fa = __uint_as_float(a), fb = __uint_as_float(b);
    operands[2 * i] = a;
    operands[2 * i + 1] = b;
    results[2 * i] = __float_as_uint(fa / fb);
    results[2 * i + 1] = __float_as_uint(sqrtExact(__uint_as_float(a & 0x7fffffffu)));
}

// One matrix-core product with the operand maps of mfma_i8.h: a (32 x 16) . b (16 x 32), both int8 and row-major, to the
// row-major 32 x 32 int32 tile `out`.  One wave.
__global__ void cvttmi_selftest_mfma_i8_kernel(const int8_t *__restrict__ a, const int8_t *__restrict__ b, int *__restrict__ out)
{
    const int l = threadIdx.x, rc = l & 31, kh = l >> 5;
    u64 av = 0, bv = 0;
#pragma unroll
    for (int t = 0; t < 8; t++)
    {
        av |= (u64)(uint8_t)a[rc * 16 + 8 * kh + t] << (8 * t);
        bv |= (u64)(uint8_t)b[(8 * kh + t) * 32 + rc] << (8 * t);
    }
    v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    acc = mfmaI8(av, bv, acc);
#pragma unroll
    for (int r = 0; r < 16; r++)
        out[mfmaRowOf(r, kh) * 32 + rc] = acc[r];
}

// endpointByte (cvtt_kernel_common.h) against (int)clampRound(x, 255.0f) on every one of the 2^32 binary32 bit patterns -- NaNs,
// both infinities, both zeros and denormals included.  2^20 threads, 2^12 patterns each.  result[0] += the patterns that differ,
// result[1] = min(the lowest such pattern).
__global__ void cvttmi_selftest_endpoint_byte_kernel(unsigned long long *__restrict__ result)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mine = 0, first = 0xffffffffull;
    for (u32 j = 0; j < 4096u; j++)
    {
        const u32 bits = (j << 20) | t;
        const float x = __uint_as_float(bits);
        if (endpointByte(x) != (int)clampRound(x, 255.0f))
        {
            mine++;
            first = first < bits ? first : bits;
        }
    }
    if (mine)
    {
        atomicAdd(&result[0], mine);
        atomicMin(&result[1], first);
    }
}
} // namespace

// d_result: two 64-bit words, {0, 0xffffffff} on entry.
extern "C" hipError_t cvttmi_launch_selftest_endpoint_byte(void *d_result, hipStream_t stream)
{
    hipLaunchKernelGGL(cvttmi_selftest_endpoint_byte_kernel, dim3(4096), dim3(256), 0, stream, (unsigned long long *)d_result);
    return hipGetLastError();
}

extern "C" hipError_t cvttmi_launch_selftest_mfma_i8(const void *d_a, const void *d_b, void *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(cvttmi_selftest_mfma_i8_kernel, dim3(1), dim3(64), 0, stream, (const int8_t *)d_a, (const int8_t *)d_b, (int *)d_out);
    return hipGetLastError();
}

extern "C" hipError_t cvttmi_launch_selftest(uint64_t seed, uint64_t first, uint32_t count, void *d_operands, void *d_results,
                                             hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(cvttmi_selftest_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, seed, first, count,
                       (u32 *)d_operands, (u32 *)d_results);
    return hipGetLastError();
}
