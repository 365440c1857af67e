// v_mfma_i32_32x32x16_i8: D (32 x 32, int32) = A (32 x 16, int8) . B (16 x 32, int8) + C, one wave.
// The operand maps, in one place for the kernel that relies on them (bc7_kernel.hip, the first-tier partition sums) and the
// self-test that pins them (selftest_kernel.hip, cvttmi_selftest_mfma_i8; tests/test_mfma_i8_map_gpu.py):
//   A   lane l holds row    l & 31, K indexes 8 * (l >> 5) .. 8 * (l >> 5) + 7, one per byte of the 64-bit operand, lowest first
//   B   lane l holds column l & 31, the same K indexes
//   C/D lane l, register r: column l & 31, row (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
#pragma once
#include "cvtt_kernel_common.h"

typedef int v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ v16i mfmaI8(u64 a, u64 b, v16i c)
{
    return __builtin_amdgcn_mfma_i32_32x32x16_i8((long)a, (long)b, c, 0, 0, 0);
}

__device__ __forceinline__ constexpr int mfmaRowOf(int reg, int laneHalf) { return (reg & 3) + 8 * (reg >> 2) + 4 * laneHalf; }
