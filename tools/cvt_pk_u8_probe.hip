// Probe for the last-round index clamp of the BC7 dual-plane search (cvtt_kernel_common.h: clampHigh): on every one of the 2^32
// binary32 bit patterns x and for hi = 3, 7, 15 (the index ranges of modes 4 / 5) and 255, the byte that
//     v_cvt_pk_u8_f32(fminf(x, hi))
// files must equal (u32)rintf(fmaxf(fminf(x, hi), 0.0f)), the byte the full clampRound sequence gives -- NaN, both infinities,
// both zeros and denormals included.  Prints the number of mismatches per hi and the first mismatching pattern; exit status 0 only
// when there is none.
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/cvt_pk_u8_probe.hip -o cvt_pk_u8_probe && ./cvt_pk_u8_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

__global__ void probe(float hi, unsigned long long *bad, unsigned *firstBad)
{
    // 2^20 threads x 2^12 patterns each
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mine = 0;
    for (uint32_t j = 0; j < 4096u; j++)
    {
        const uint32_t bits = (j << 20) | t;
        const float x = __uint_as_float(bits);
        const float c = fminf(x, hi);
        const uint32_t want = (uint32_t)rintf(fmaxf(c, 0.0f));
        // into byte 1 of a word of ones: the neighbours must survive, too
        const uint32_t w = __builtin_amdgcn_cvt_pk_u8_f32(c, 1u, 0xffffffffu);
        if (w != (0xffff00ffu | (want << 8)))
        {
            if (mine == 0)
                atomicMin(firstBad, bits);
            mine++;
        }
    }
    if (mine)
        atomicAdd(bad, mine);
}

int main()
{
    unsigned long long *dBad;
    unsigned *dFirst;
    if (hipMalloc(&dBad, sizeof(*dBad)) != hipSuccess || hipMalloc(&dFirst, sizeof(*dFirst)) != hipSuccess)
    {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    int rc = 0;
    const float his[4] = {3.0f, 7.0f, 15.0f, 255.0f};
    for (int i = 0; i < 4; i++)
    {
        unsigned long long bad = 0;
        unsigned first = 0xffffffffu;
        hipMemcpy(dBad, &bad, sizeof(bad), hipMemcpyHostToDevice);
        hipMemcpy(dFirst, &first, sizeof(first), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(probe, dim3(4096), dim3(256), 0, 0, his[i], dBad, dFirst);
        if (hipDeviceSynchronize() != hipSuccess)
        {
            fprintf(stderr, "kernel failed\n");
            return 2;
        }
        hipMemcpy(&bad, dBad, sizeof(bad), hipMemcpyDeviceToHost);
        hipMemcpy(&first, dFirst, sizeof(first), hipMemcpyDeviceToHost);
        printf("hi = %3.0f: %llu of 4294967296 patterns differ", his[i], bad);
        if (bad)
            printf(" (lowest: 0x%08x)", first);
        printf("\n");
        if (bad)
            rc = 1;
    }
    hipFree(dBad);
    hipFree(dFirst);
    return rc;
}
