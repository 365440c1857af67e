// Host references of the lane-test library, compiled with the product's host flags.  What stands for an SSE2 instruction on the
// device is computed here with that instruction, operands in the order the reference's ParallelMath.h gives them; the integer
// and float rules of the resampling headers are restated in plain C++, every float operation rounded on its own
// (-ffp-contract=off).  Each sweep reference fills the checksums of chunks [chunk0, chunk0 + count) -- the caller spreads the 2^20
// chunks over its threads -- and, where `full` is given, the 4096 results of each of them.
#include <emmintrin.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "lanetest_checksum.h"

namespace
{
inline float asFloat(uint32_t bits)
{
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

inline uint32_t asBits(float f)
{
    uint32_t bits;
    memcpy(&bits, &f, 4);
    return bits;
}

template <class F>
int sweep(F f, uint32_t chunk0, uint32_t count, uint64_t *sums, uint32_t *full)
{
    if (chunk0 > lanetest::kChunks || count > lanetest::kChunks - chunk0)
        return -1;
    for (uint32_t c = 0; c < count; c++)
    {
        const uint32_t first = (chunk0 + c) << 12;
        uint64_t acc = 0;
        for (uint32_t j = 0; j < lanetest::kChunk; j++)
        {
            const uint32_t r = f(first | j);
            acc += lanetest::term(r, j);
            if (full)
                full[(size_t)c * lanetest::kChunk + j] = r;
        }
        if (sums)
            sums[c] = acc;
    }
    return 0;
}

// ParallelMath::Clamp(v, 0, hi) then RoundAndConvertToU15: MAXPS(MINPS(v, hi), 0), CVTPS2DQ under the default rounding mode
inline int clampConvert(float v, float hi)
{
    const __m128 c = _mm_max_ps(_mm_min_ps(_mm_set1_ps(v), _mm_set1_ps(hi)), _mm_set1_ps(0.0f));
    return _mm_cvtsi128_si32(_mm_cvtps_epi32(c));
}
} // namespace

// the integer the reference converts to (asFloat = 0), or that integer as a float's bits (asFloat = 1)
extern "C" int lanetest_ref_clamp_convert(float hi, int asFloatBits, uint32_t chunk0, uint32_t count, uint64_t *sums, uint32_t *full)
{
    if (asFloatBits)
        return sweep([hi](uint32_t bits) { return asBits((float)clampConvert(asFloat(bits), hi)); }, chunk0, count, sums, full);
    return sweep([hi](uint32_t bits) { return (uint32_t)clampConvert(asFloat(bits), hi); }, chunk0, count, sums, full);
}

// v == 0 ? 1 : v, the bits of v kept (a NaN too)
extern "C" int lanetest_ref_safe_denom(uint32_t chunk0, uint32_t count, uint64_t *sums, uint32_t *full)
{
    return sweep([](uint32_t bits) { return (bits & 0x7fffffffu) == 0 ? 0x3f800000u : bits; }, chunk0, count, sums, full);
}

// clamp((s + 2^17) >> 18, 0 ... 255 or -128 ... 127) as a byte, the sum taken in 64 bits: the shift, then the clamp
extern "C" int lanetest_ref_plain_byte(int isSnorm, uint32_t chunk0, uint32_t count, uint64_t *sums, uint32_t *full)
{
    if (isSnorm)
        return sweep([](uint32_t bits) {
            const int64_t q = ((int64_t)(int32_t)bits + (1 << 17)) >> 18;
            return (uint32_t)(q < -128 ? -128 : q > 127 ? 127 : q) & 255u; }, chunk0, count, sums, full);
    return sweep([](uint32_t bits) {
        const int64_t q = ((int64_t)(int32_t)bits + (1 << 17)) >> 18;
        return (uint32_t)(q < 0 ? 0 : q > 255 ? 255 : q); }, chunk0, count, sums, full);
}

// The byte of a component q of a unit normal, |q| <= 1 + 2^-20: floor(q * 127.5 + 128) clamped to 0 ... 255, or floor(q * 127 + 0.5)
// clamped to -127 ... 127 as an int8's bits.  The product, the sum and the floor are three binary32 operations.  0 for every
// other pattern.
extern "C" int lanetest_ref_normal_byte(int isSnorm, uint32_t chunk0, uint32_t count, uint64_t *sums, uint32_t *full)
{
    if (isSnorm)
        return sweep([](uint32_t bits) {
            if ((bits & 0x7fffffffu) > 0x3f800008u)
                return 0u;
            const float product = asFloat(bits) * 127.0f;
            const float sum = product + 0.5f;
            const int r = (int)floorf(sum);
            return (uint32_t)(r < -127 ? -127 : r > 127 ? 127 : r) & 255u; }, chunk0, count, sums, full);
    return sweep([](uint32_t bits) {
        if ((bits & 0x7fffffffu) > 0x3f800008u)
            return 0u;
        const float product = asFloat(bits) * 127.5f;
        const float sum = product + 128.0f;
        const int r = (int)floorf(sum);
        return (uint32_t)(r < 0 ? 0 : r > 255 ? 255 : r); }, chunk0, count, sums, full);
}

// MINSS / MAXSS element by element, operands in ParallelMath's order: Min(a, b) = _mm_min_ps(a, b)
extern "C" void lanetest_ref_sse_min(const float *a, const float *b, uint32_t n, float *out)
{
    for (uint32_t i = 0; i < n; i++)
        _mm_store_ss(&out[i], _mm_min_ss(_mm_load_ss(&a[i]), _mm_load_ss(&b[i])));
}

extern "C" void lanetest_ref_sse_max(const float *a, const float *b, uint32_t n, float *out)
{
    for (uint32_t i = 0; i < n; i++)
        _mm_store_ss(&out[i], _mm_max_ss(_mm_load_ss(&a[i]), _mm_load_ss(&b[i])));
}
