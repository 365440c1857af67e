// Probe for the lower index clamp of the BC7 dual-plane search's non-last refine rounds (bc7_dual.h, evalDual<true>): on every
// one of the 2^32 binary32 bit patterns v and for hi = 3 and 7 (the index ranges of modes 4 / 5), with c = fminf(v, hi) the
// upper clamp (clampHigh), the index that the round files and weights the refiner with,
//     old form       rintf(fmaxf(c, 0.0f))       where the compiler, not seeing that c comes from a v_min_f32, emits
//                                                v_max_f32 c, c, c ahead of v_max_f32 c, 0, c
//     one v_max      rintf(v_max_f32(0, c))      the second instruction of the pair alone (inline assembly)
//     round first    fmaxf(rintf(c), 0.0f)       v_rndne_f32 ahead of the same v_max_f32, both in one basic block
// must be the same 32 bits -- the sign of a zero included, NaN, both infinities and denormals among the inputs -- and
// v_cvt_pk_u8_f32 must file the same byte from each.  The old form is compiled as the kernel has it: the upper clamp on one
// side of a branch the compiler cannot fold, the lower clamp on the other.  Prints the number of mismatches per form and hi
// and the lowest mismatching pattern; exit status 0 only when there is none.
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/clamp_low_probe.hip -o clamp_low_probe && ./clamp_low_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

__device__ __forceinline__ float oneMax(float c)
{
    float r;
    asm("v_max_f32_e32 %0, 0, %1" : "=v"(r) : "v"(c));
    return r;
}

// bad[0] / first[0]: one v_max against the old form; bad[1] / first[1]: round first against the old form
__global__ void probe(float hi, int notLast, unsigned long long *bad, unsigned *first)
{
    // 2^20 threads x 2^12 patterns each
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mine[2] = {0, 0};
    for (uint32_t j = 0; j < 4096u; j++)
    {
        const uint32_t bits = (j << 20) | t;
        const float v = __uint_as_float(bits);
        const float c = fminf(v, hi);
        float old = c;
        if (notLast) // a kernel argument, always 1: the lower clamp of the old form sits in a block of its own
            old = rintf(fmaxf(old, 0.0f));
        const float form[2] = {rintf(oneMax(c)), fmaxf(rintf(c), 0.0f)};
        const uint32_t wOld = __builtin_amdgcn_cvt_pk_u8_f32(old, 1u, 0xffffffffu);
        for (int f = 0; f < 2; f++)
        {
            const uint32_t w = __builtin_amdgcn_cvt_pk_u8_f32(form[f], 1u, 0xffffffffu);
            if (__float_as_uint(form[f]) != __float_as_uint(old) || w != wOld)
            {
                if (mine[f] == 0)
                    atomicMin(first + f, bits);
                mine[f]++;
            }
        }
    }
    for (int f = 0; f < 2; f++)
        if (mine[f])
            atomicAdd(bad + f, mine[f]);
}

int main()
{
    unsigned long long *dBad;
    unsigned *dFirst;
    if (hipMalloc(&dBad, 2 * sizeof(*dBad)) != hipSuccess || hipMalloc(&dFirst, 2 * sizeof(*dFirst)) != hipSuccess)
    {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    int rc = 0;
    const float his[2] = {3.0f, 7.0f};
    const char *names[2] = {"one v_max  ", "round first"};
    for (int i = 0; i < 2; i++)
    {
        unsigned long long bad[2] = {0, 0};
        unsigned first[2] = {0xffffffffu, 0xffffffffu};
        hipMemcpy(dBad, bad, sizeof(bad), hipMemcpyHostToDevice);
        hipMemcpy(dFirst, first, sizeof(first), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(probe, dim3(4096), dim3(256), 0, 0, his[i], 1, dBad, dFirst);
        if (hipDeviceSynchronize() != hipSuccess)
        {
            fprintf(stderr, "kernel failed\n");
            return 2;
        }
        hipMemcpy(bad, dBad, sizeof(bad), hipMemcpyDeviceToHost);
        hipMemcpy(first, dFirst, sizeof(first), hipMemcpyDeviceToHost);
        for (int f = 0; f < 2; f++)
        {
            printf("hi = %1.0f, %s: %llu of 4294967296 patterns differ from the old form", his[i], names[f], bad[f]);
            if (bad[f])
                printf(" (lowest: 0x%08x)", first[f]);
            printf("\n");
            if (bad[f])
                rc = 1;
        }
    }
    hipFree(dBad);
    hipFree(dFirst);
    return rc;
}
