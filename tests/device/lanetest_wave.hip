// Lane-test kernels over cvtt_kernel_common.h and etc2_wave.h (and the quad moves of bc6h_quant.h): the small exact
// divisions, the v_min_f32 of loaded values, every lane move and the wave-wide argmin.  The functions are the product
// headers' own, compiled with the product's device flags.
#include "cvtt_kernel_common.h"
#include <hip/hip_fp16.h>
#include "bc6h_quant.h"
#include "etc2_wave.h"
#include "lanetest_device.h"

namespace
{
// udivSmall(n, d) against n / d for every 0 <= n < 2^16, 1 <= d < 2^12: a thread takes one d and 256 consecutive n.  An
// input's number: d << 16 | n.
__global__ void udivSmallKernel(unsigned long long *__restrict__ result)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x; // 4096 d x 256 slices of n = 2^20 threads
    const int d = (int)(t >> 8);
    const int n0 = (int)(t & 255u) << 8;
    if (d == 0)
        return;
    unsigned long long mine = 0, first = ~0ull;
    for (int k = 0; k < 256; k++)
    {
        const int n = n0 + k;
        if (udivSmall(n, d) != n / d)
        {
            const unsigned long long id = ((unsigned long long)d << 16) | (unsigned long long)n;
            mine++;
            first = first < id ? first : id;
        }
    }
    lanetestReport(result, mine, first);
}

__global__ void udivSmall20Kernel(int *__restrict__ out)
{
    const int d = (int)threadIdx.x + 1; // 128 threads: d = 1 ... 128
    out[threadIdx.x] = udivSmall20(d);
}

__global__ void minLoadedKernel(const float *__restrict__ a, const float *__restrict__ b, u32 n, float *__restrict__ out)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = minLoaded(a[i], b[i]);
}

// Every lane move on one wave's 64 values.  Row r of `out` (64 words each):
//   0-5 xorLane(int, 1 << r)     6-11 xorLaneI<1 << (r - 6)>     12-17 xorLaneF<1 << (r - 12)> (the bits)
//   18-23 xorLane(float, ...), 24-29 xorLane(unsigned, ...)
//   30 quadPerm<0xb1>  31 quadPerm<0x4e>  32-35 quadBcast<0..3>  36 quadOr  37 quadMin (of the bits as a float)
//   38 / 39 groupBits(ballot of bit 0 of the value, lane): every lane's view
//   40 uniU  41 uniI  42 uniF  43 laneI(v, pick)  44 laneF(v, pick)
const int kLaneRows = 45;
__global__ void laneMovesKernel(const u32 *__restrict__ in, int pick, u32 *__restrict__ out)
{
    const int l = (int)threadIdx.x;
    const u32 v = in[l];
    const float f = __uint_as_float(v);
    u32 *o = out + l;
#pragma unroll
    for (int r = 0; r < 6; r++)
    {
        o[64 * r] = (u32)xorLane((int)v, 1 << r);
        o[64 * (18 + r)] = __float_as_uint(xorLane(f, 1 << r));
        o[64 * (24 + r)] = xorLane(v, 1 << r);
    }
    o[64 * 6] = (u32)xorLaneI<1>((int)v);
    o[64 * 7] = (u32)xorLaneI<2>((int)v);
    o[64 * 8] = (u32)xorLaneI<4>((int)v);
    o[64 * 9] = (u32)xorLaneI<8>((int)v);
    o[64 * 10] = (u32)xorLaneI<16>((int)v);
    o[64 * 11] = (u32)xorLaneI<32>((int)v);
    o[64 * 12] = __float_as_uint(xorLaneF<1>(f));
    o[64 * 13] = __float_as_uint(xorLaneF<2>(f));
    o[64 * 14] = __float_as_uint(xorLaneF<4>(f));
    o[64 * 15] = __float_as_uint(xorLaneF<8>(f));
    o[64 * 16] = __float_as_uint(xorLaneF<16>(f));
    o[64 * 17] = __float_as_uint(xorLaneF<32>(f));
    o[64 * 30] = quadPerm<0xb1>(v);
    o[64 * 31] = quadPerm<0x4e>(v);
    o[64 * 32] = quadBcast<0>(v);
    o[64 * 33] = quadBcast<1>(v);
    o[64 * 34] = quadBcast<2>(v);
    o[64 * 35] = quadBcast<3>(v);
    o[64 * 36] = quadOr(v);
    o[64 * 37] = __float_as_uint(quadMin(f));
    const u64 ballot = __ballot((v & 1u) != 0);
    o[64 * 38] = groupBits(ballot, l);
    o[64 * 39] = groupBits(~ballot, l);
    o[64 * 40] = uniU(v);
    o[64 * 41] = (u32)uniI((int)v);
    o[64 * 42] = __float_as_uint(uniF(f));
    o[64 * 43] = (u32)laneI((int)v, pick);
    o[64 * 44] = __float_as_uint(laneF(f, pick));
}

// one wave per case: 64 (err, id) in, every lane's (err, id) out
__global__ void waveArgminKernel(const float *__restrict__ err, const int *__restrict__ id, u32 *__restrict__ outErr, int *__restrict__ outId)
{
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    float e = err[i];
    int k = id[i];
    waveArgmin(e, k);
    outErr[i] = __float_as_uint(e);
    outId[i] = k;
}
} // namespace

extern "C" hipError_t lanetest_udiv_small(void *d_result, hipStream_t stream)
{
    hipLaunchKernelGGL(udivSmallKernel, dim3(4096), dim3(256), 0, stream, (unsigned long long *)d_result);
    return hipGetLastError();
}

// d_out: 128 words, ceil(2^20 / d) for d = 1 ... 128
extern "C" hipError_t lanetest_udiv_small20(void *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(udivSmall20Kernel, dim3(1), dim3(128), 0, stream, (int *)d_out);
    return hipGetLastError();
}

extern "C" hipError_t lanetest_min_loaded(const void *d_a, const void *d_b, uint32_t n, void *d_out, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(minLoadedKernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, (const float *)d_a, (const float *)d_b, n, (float *)d_out);
    return hipGetLastError();
}

extern "C" int lanetest_lane_rows(void) { return kLaneRows; }

// d_in: 64 words; d_out: lanetest_lane_rows() x 64 words; pick: the lane laneI / laneF read, 0 ... 63
extern "C" hipError_t lanetest_lane_moves(const void *d_in, int pick, void *d_out, hipStream_t stream)
{
    if (pick < 0 || pick > 63)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(laneMovesKernel, dim3(1), dim3(64), 0, stream, (const u32 *)d_in, pick, (u32 *)d_out);
    return hipGetLastError();
}

// cases x 64 values each way
extern "C" hipError_t lanetest_wave_argmin(const void *d_err, const void *d_id, uint32_t cases, void *d_outErr, void *d_outId, hipStream_t stream)
{
    if (cases == 0)
        return hipSuccess;
    hipLaunchKernelGGL(waveArgminKernel, dim3(cases), dim3(64), 0, stream, (const float *)d_err, (const int *)d_id, (u32 *)d_outErr, (int *)d_outId);
    return hipGetLastError();
}
