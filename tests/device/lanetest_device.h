// The launch shapes of the lane-test library (tests/device/): a sweep of all 2^32 inputs of a function as 2^20 chunk
// checksums, one chunk's results in full, and the report of a sweep that compares on the device.  Test code only; nothing
// here is linked into the product.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lanetest_checksum.h"

namespace
{
// sums[t] = the checksum of chunk t.  4096 workgroups of 256 lanes: exactly 2^20 threads, one per chunk.
template <class F>
__global__ void lanetestSumsKernel(F f, uint64_t *__restrict__ sums)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t acc = 0;
    for (uint32_t j = 0; j < lanetest::kChunk; j++)
        acc += lanetest::term(f((t << 12) | j), j);
    sums[t] = acc;
}

// out[j] = f(chunk << 12 | j), j < 4096: 16 workgroups of 256 lanes
template <class F>
__global__ void lanetestChunkKernel(F f, uint32_t chunk, uint32_t *__restrict__ out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    out[j] = f((chunk << 12) | j);
}

template <class F>
hipError_t lanetestSums(F f, void *d_sums, hipStream_t stream)
{
    hipLaunchKernelGGL(lanetestSumsKernel<F>, dim3(4096), dim3(256), 0, stream, f, (uint64_t *)d_sums);
    return hipGetLastError();
}

template <class F>
hipError_t lanetestChunk(F f, uint32_t chunk, void *d_out, hipStream_t stream)
{
    if (chunk >= lanetest::kChunks)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lanetestChunkKernel<F>, dim3(lanetest::kChunk / 256), dim3(256), 0, stream, f, chunk, (uint32_t *)d_out);
    return hipGetLastError();
}

// A sweep that compares on the device: result[0] += the inputs that differ, result[1] = min(the lowest such input, as the
// sweep numbers its inputs).  {0, ~0} on entry.
__device__ __forceinline__ void lanetestReport(unsigned long long *result, unsigned long long mine, unsigned long long first)
{
    if (mine)
    {
        atomicAdd(&result[0], mine);
        atomicMin(&result[1], first);
    }
}
} // namespace

// lanetest_<name>(hi, d_sums, stream): 2^20 checksums (8 MiB); lanetest_<name>_chunk(hi, chunk, d_out, stream): the 4096
// results of one chunk.  `expr` sees the input as `bits` and as the float `v`, and the parameter `hi`.
#define LANETEST_SWEEP32(name, expr)                                                                              \
    namespace                                                                                                     \
    {                                                                                                             \
    struct name##Fn                                                                                               \
    {                                                                                                             \
        float hi;                                                                                                 \
        __device__ __forceinline__ uint32_t operator()(uint32_t bits) const                                       \
        {                                                                                                         \
            const float v = __uint_as_float(bits);                                                                \
            (void)v;                                                                                              \
            return (uint32_t)(expr);                                                                              \
        }                                                                                                         \
    };                                                                                                            \
    }                                                                                                             \
    extern "C" hipError_t lanetest_##name(float hi, void *d_sums, hipStream_t stream)                             \
    {                                                                                                             \
        return lanetestSums(name##Fn{hi}, d_sums, stream);                                                        \
    }                                                                                                             \
    extern "C" hipError_t lanetest_##name##_chunk(float hi, uint32_t chunk, void *d_out, hipStream_t stream)      \
    {                                                                                                             \
        return lanetestChunk(name##Fn{hi}, chunk, d_out, stream);                                                 \
    }
