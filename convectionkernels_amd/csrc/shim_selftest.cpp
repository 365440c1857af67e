// The three self-tests of the library: diagnostics that run a small kernel and compare on the host (not part of include/, except
// cvttmi_selftest_arith).
#include "shim_internal.h"

#include <vector>
#include <xmmintrin.h>

using namespace cvtt_shim;

extern "C"
{
    int cvttmi_selftest_arith(cvttmi_context *ctx, uint64_t count, uint64_t seed, uint64_t *divMismatches, uint64_t *sqrtMismatches)
    {
        if (!ctx || !divMismatches || !sqrtMismatches)
            return CVTTMI_E_INVALID;
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess)
            return fail(ctx, CVTTMI_E_NO_DEVICE, "hipSetDevice", e);
        const uint32_t chunk = 1u << 20;
        cvtt_owned::DeviceBuffer ops8, res8; // freed on every way out
        if (ops8.reserve(chunk * 8) != hipSuccess || res8.reserve(chunk * 8) != hipSuccess)
            return fail(ctx, CVTTMI_E_HIP, "hipMalloc (selftest)");
        uint32_t *const dOps = ops8.as<uint32_t>(), *const dRes = res8.as<uint32_t>();
        std::vector<uint32_t> ops(chunk * 2), res(chunk * 2);
        uint64_t badDiv = 0, badSqrt = 0;
        for (uint64_t first = 0; first < count; first += chunk)
        {
            const uint32_t n = static_cast<uint32_t>(count - first < chunk ? count - first : chunk);
            e = cvttmi_launch_selftest(seed, first, n, dOps, dRes, NULL);
            if (e == hipSuccess) e = hipMemcpy(ops.data(), dOps, (size_t)n * 8, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(res.data(), dRes, (size_t)n * 8, hipMemcpyDeviceToHost);
            if (e != hipSuccess)
                return fail(ctx, CVTTMI_E_HIP, "selftest kernel", e);
            for (uint32_t i = 0; i < n; i++)
            {
                float a, b;
                memcpy(&a, &ops[2 * i], 4);
                memcpy(&b, &ops[2 * i + 1], 4);
                const float q = _mm_cvtss_f32(_mm_div_ss(_mm_set_ss(a), _mm_set_ss(b)));
                uint32_t absBits = ops[2 * i] & 0x7fffffffu;
                float absA;
                memcpy(&absA, &absBits, 4);
                const float r = _mm_cvtss_f32(_mm_sqrt_ss(_mm_set_ss(absA)));
                uint32_t qb, rb;
                memcpy(&qb, &q, 4);
                memcpy(&rb, &r, 4);
                const bool qNan = (qb & 0x7fffffffu) > 0x7f800000u, gNan = (res[2 * i] & 0x7fffffffu) > 0x7f800000u;
                if (!(qNan && gNan) && qb != res[2 * i])
                    badDiv++;
                if (rb != res[2 * i + 1])
                    badSqrt++;
            }
        }
        *divMismatches = badDiv;
        *sqrtMismatches = badSqrt;
        return CVTTMI_OK;
    }

    // Diagnostic (tests/test_mfma_i8_map_gpu.py, not part of include/): one matrix-core product with the operand maps the BC7
    // first-tier sums rely on (mfma_i8.h).  a: 32 x 16, b: 16 x 32, both int8 and row-major; out: the 32 x 32 int32 tile,
    // row-major.  Host pointers.
    int cvttmi_selftest_mfma_i8(cvttmi_context *ctx, const int8_t *a, const int8_t *b, int32_t *out)
    {
        if (!ctx || !a || !b || !out)
            return CVTTMI_E_INVALID;
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess)
            return fail(ctx, CVTTMI_E_NO_DEVICE, "hipSetDevice", e);
        cvtt_owned::DeviceBuffer buffer;
        if (buffer.reserve(512 + 512 + 4096) != hipSuccess)
            return fail(ctx, CVTTMI_E_HIP, "hipMalloc (selftest)");
        char *const d = buffer.as<char>();
        e = hipMemcpy(d, a, 512, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + 512, b, 512, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = cvttmi_launch_selftest_mfma_i8(d, d + 512, d + 1024, NULL);
        if (e == hipSuccess) e = hipMemcpy(out, d + 1024, 4096, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return fail(ctx, CVTTMI_E_HIP, "selftest (mfma i8) kernel", e);
        return CVTTMI_OK;
    }

    // Diagnostic (tests/test_endpoint_byte_identity_gpu.py, not part of include/): the two-instruction endpoint byte of the BC7
    // kernels (cvtt_kernel_common.h: endpointByte) against (int)clampRound(x, 255) on all 2^32 binary32 bit patterns, on the
    // device.  mismatches: how many patterns differ; firstMismatch: the lowest of them (0xffffffff when there is none).
    int cvttmi_selftest_endpoint_byte(cvttmi_context *ctx, uint64_t *mismatches, uint32_t *firstMismatch)
    {
        if (!ctx || !mismatches || !firstMismatch)
            return CVTTMI_E_INVALID;
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess)
            return fail(ctx, CVTTMI_E_NO_DEVICE, "hipSetDevice", e);
        cvtt_owned::DeviceBuffer buffer;
        if (buffer.reserve(16) != hipSuccess)
            return fail(ctx, CVTTMI_E_HIP, "hipMalloc (selftest)");
        unsigned long long *const d = buffer.as<unsigned long long>();
        unsigned long long r[2] = {0ull, 0xffffffffull};
        e = hipMemcpy(d, r, 16, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = cvttmi_launch_selftest_endpoint_byte(d, NULL);
        if (e == hipSuccess) e = hipMemcpy(r, d, 16, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return fail(ctx, CVTTMI_E_HIP, "selftest (endpoint byte) kernel", e);
        *mismatches = r[0];
        *firstMismatch = static_cast<uint32_t>(r[1]);
        return CVTTMI_OK;
    }
}
