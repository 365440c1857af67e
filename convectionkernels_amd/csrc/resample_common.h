// What the resampling kernels share (mip_filter_kernel.hip: the 2x2 filters, the box among them; mip_resample_kernel.hip: the mip
// kernels wider than 2x2; resize_kernel.hip: any size): the rules and wraps of include/cvtt_mi355x.h's filter word, the value a
// texel's channel contributes under a rule and the byte a rule's sum or quotient becomes, the sRGB tables in LDS, the walk along a
// wrapped axis, and the one list of the (pixel kind, rule) pairs that exist.  Every mip and resize kernel file includes it.
#pragma once
#include "mip_common.h"
#include "../../include/cvtt_mi355x.h"
#include <type_traits>

#define CVTT_SRGB_TABLE __device__ const __attribute__((aligned(16))) // (the byte table is copied a word at a time)
#include "srgb_tables.h"

namespace
{
// the rule, alpha-weight and wrap fields of a filter word, and the pixel kinds, as the public header numbers them
enum
{
    kPlain = CVTTMI_MIP_FILTER_BOX, // under a kernel: the plain rule
    kSrgb = CVTTMI_MIP_FILTER_SRGB,
    kNormal = CVTTMI_MIP_FILTER_NORMAL,
    kAlphaWeighted = CVTTMI_MIP_FILTER_ALPHA_WEIGHTED,
    kWrapRepeat = CVTTMI_MIP_WRAP_REPEAT,
    kWrapMirror = CVTTMI_MIP_WRAP_MIRROR,
    kHdrNonnegative = CVTTMI_MIP_HDR_NONNEGATIVE,
    kHdrSigned = CVTTMI_MIP_HDR_SIGNED
};
static_assert(kRGBA8 == CVTTMI_PIXELS_RGBA8 && kRGBA16F == CVTTMI_PIXELS_RGBA16F && kRGBA8Snorm == CVTTMI_PIXELS_RGBA8_SNORM, "mip_common.h");

inline bool wrapOk(uint32_t wrap) // clamp or one flag
{
    return wrap == 0 || wrap == kWrapRepeat || wrap == kWrapMirror;
}

// ---- the (pixel kind, rule) pairs that exist ----
// f(kind, rule), both std::integral_constant, for the pair a call names; hipErrorInvalidValue where there is no such pair.  Under
// a kernel and in a resize RGBA8 takes the plain rule, SRGB and NORMAL, RGBA8_SNORM the plain rule and NORMAL, RGBA16F the plain
// rule (in float, with a range: "RGBA16F" below; the kind is a parameter of the same kernel templates).  This is the only place
// that lists the pairs: cvttmi_resize_entry_bytes answers "is there such a pair" for the host through it.
template <class F>
hipError_t withKindRule(int kind, uint32_t rule, F f)
{
    typedef std::integral_constant<int, kRGBA8> U8;
    typedef std::integral_constant<int, kRGBA8Snorm> S8;
    if (kind == kRGBA16F && rule == kPlain)
        return f(std::integral_constant<int, kRGBA16F>(), std::integral_constant<int, kPlain>());
    if (kind == kRGBA8 && rule == kPlain)
        return f(U8(), std::integral_constant<int, kPlain>());
    if (kind == kRGBA8 && rule == kSrgb)
        return f(U8(), std::integral_constant<int, kSrgb>());
    if (kind == kRGBA8 && rule == kNormal)
        return f(U8(), std::integral_constant<int, kNormal>());
    if (kind == kRGBA8Snorm && rule == kPlain)
        return f(S8(), std::integral_constant<int, kPlain>());
    if (kind == kRGBA8Snorm && rule == kNormal)
        return f(S8(), std::integral_constant<int, kNormal>());
    return hipErrorInvalidValue;
}

// The 2x2 filters: the same pairs (the plain rule is the box), and ALPHA_WEIGHTED on the BOX and SRGB of RGBA8.  f(kind, filter).
template <class F>
hipError_t withKindFilter(int kind, uint32_t filter, F f)
{
    typedef std::integral_constant<int, kRGBA8> U8;
    if (kind == kRGBA8 && filter == kAlphaWeighted)
        return f(U8(), std::integral_constant<int, kAlphaWeighted>());
    if (kind == kRGBA8 && filter == (kSrgb | kAlphaWeighted))
        return f(U8(), std::integral_constant<int, kSrgb | kAlphaWeighted>());
    return withKindRule(kind, filter, f);
}

// ---- the sRGB tables in LDS (tools/gen_srgb_tables.py) ----
// encode(S) = number of thresholds U[k] <= S: one byte of coarse[S >> 6] = encode(S with its low six bits cleared) and one
// threshold -- U's steps are above 64, so S passes at most one threshold more than its bucket's start.  The mip kernels carry the
// three tables in one struct (5 632 B); resize splits them, lin (512 B) for its horizontal pass, the other two (5 120 B) for its
// vertical one.
struct SrgbTables
{
    uint32_t next[256]; // [c] = U[c + 1], the threshold above code c; [255] = no sum reaches it
    uint16_t lin[256];
    uint8_t coarse[4096];
};

struct SrgbEncodeTables
{
    uint32_t next[256];
    uint8_t coarse[4096];
};

// the workgroup's copy of the tables, made by its `lanes` lanes, this one being `lane`: every lane comes here, the ones without a
// texel too, and the caller synchronises.  (The arguments in this order: the other way round the 2x2 kernels schedule differently.)
__device__ __forceinline__ void loadSrgbTables(SrgbTables &t, uint32_t lanes, uint32_t lane)
{
    for (uint32_t i = lane; i < 256u; i += lanes)
    {
        t.next[i] = i < 255u ? k_srgbThresholds[i] : 0xffffffffu;
        t.lin[i] = k_srgbToLinear[i];
    }
    for (uint32_t i = lane; i < 1024u; i += lanes)
        reinterpret_cast<uint32_t *>(t.coarse)[i] = reinterpret_cast<const uint32_t *>(k_srgbCoarse)[i];
}

__device__ __forceinline__ void loadLinear(uint16_t *lin) // 256 lanes
{
    lin[threadIdx.x] = k_srgbToLinear[threadIdx.x];
}

__device__ __forceinline__ void loadEncode(SrgbEncodeTables &t) // 256 lanes
{
    t.next[threadIdx.x] = threadIdx.x < 255u ? k_srgbThresholds[threadIdx.x] : 0xffffffffu;
    for (uint32_t i = threadIdx.x; i < 1024u; i += 256u)
        reinterpret_cast<uint32_t *>(t.coarse)[i] = reinterpret_cast<const uint32_t *>(k_srgbCoarse)[i];
}

template <class Tables>
__device__ __forceinline__ uint32_t srgbEncode(const Tables &t, uint32_t S) // S <= 4 * 65535
{
    const uint32_t c = t.coarse[S >> 6];
    return c + (S >= t.next[c] ? 1u : 0u);
}

// ---- a coordinate that walks along a wrapped axis of n texels ----
// `pos` is the coordinate itself (clamp), its place in the period n (repeat) or in the period 2 n of there-and-back (mirror:
// ... 1 0 | 0 1 .. n-1 | n-1 .. 0 | 0 ...).  One division where the walk starts, none per step.
struct Walk
{
    int64_t pos;
    uint32_t n, wrap;
};

__device__ __forceinline__ Walk walkFrom(int64_t i, uint32_t n, uint32_t wrap)
{
    Walk k = {i, n, wrap};
    if (wrap != 0 && (i < 0 || i >= (int64_t)n))
    {
        const uint64_t p = wrap == kWrapMirror ? 2ull * n : (uint64_t)n;
        k.pos = i >= 0 ? (int64_t)((uint64_t)i % p) : (int64_t)(p - 1u - ((uint64_t)(-i - 1) % p));
    }
    return k;
}

__device__ __forceinline__ uint32_t walkIndex(const Walk &k)
{
    if (k.wrap == kWrapMirror)
        return static_cast<uint32_t>(k.pos < (int64_t)k.n ? k.pos : 2 * (int64_t)k.n - 1 - k.pos);
    if (k.wrap == kWrapRepeat)
        return static_cast<uint32_t>(k.pos);
    return static_cast<uint32_t>(k.pos < 0 ? 0 : k.pos >= (int64_t)k.n ? (int64_t)k.n - 1 : k.pos);
}

__device__ __forceinline__ void walkStep(Walk &k)
{
    k.pos++;
    if (k.wrap != 0 && k.pos == (k.wrap == kWrapMirror ? 2 * (int64_t)k.n : (int64_t)k.n))
        k.pos = 0;
}

// ---- the rule ----
// the value channel c of a texel enters the sums with: c = 0..2 under the rule -- the byte (plain), T[byte] (SRGB, T = lin) or X
// (NORMAL) --, c = 3 the byte of channel 3, c = 4..6 (NORMAL only) the bytes of channels 0..2
template <int KIND, int RULE>
__device__ __forceinline__ int ruleValue(uint32_t texel, int c, const uint16_t *lin)
{
    const uint32_t v = (texel >> (8 * (c & 3))) & 255u;
    const int plain = KIND == kRGBA8Snorm ? static_cast<int>(static_cast<int8_t>(v)) : static_cast<int>(v);
    if (c >= 3 || RULE == kPlain)
        return plain;
    if (RULE == kSrgb)
        return lin[v];
    return KIND == kRGBA8Snorm ? max(plain, -127) : 2 * plain - 255;
}

// The last step of the plain rule: clamp((s + 2^17) >> 18, 0..255 or -128..127), written as the clamp of the sum followed by the
// shift (the same value: the shift is monotone).  Shift-then-clamp of two neighbouring channels is what the compiler turns into
// v_ashr_pk_u8_i32, whose result it then ORs into the texel whole -- on the MI355X the upper half of that register kept what
// it held before, and channel 2 and alpha of the texel came out wrong.
template <int KIND>
__device__ __forceinline__ uint32_t plainByte(int s) // s: the second pass's sum, 18 fraction bits
{
    const int t = s + (1 << 17);
    if (KIND == kRGBA8Snorm)
        return static_cast<uint32_t>(min(max(t, -(128 << 18)), (128 << 18) - 1) >> 18) & 255u;
    return static_cast<uint32_t>(min(max(t, 0), (256 << 18) - 1)) >> 18;
}

// NORMAL: the byte of q, a component of the unit vector (the product and the sum round separately: -ffp-contract=off)
template <int KIND>
__device__ __forceinline__ uint32_t normalByte(float q)
{
    const int r = KIND == kRGBA8Snorm ? min(max(static_cast<int>(floorf(q * 127.0f + 0.5f)), -127), 127)
                                      : min(max(static_cast<int>(floorf(q * 127.5f + 128.0f)), 0), 255);
    return static_cast<uint32_t>(r) & 255u;
}

// How the four sums of a second pass become a texel -- plainByte of channel 3 into bits 24..31, then channels 0..2 from plainByte,
// srgbEncode, or normalByte with the plain rule where the three sums of X are all zero -- is written out in both second passes
// (mip_resample_kernel.hip's vertical pass, resize_kernel.hip's verticalTexel): as one function here it compiled to other
// instructions in both, whichever way the sums were handed over (profiles/r24/finish_step.txt).

// ---- RGBA16F: the plain rule in binary32, with a range (CVTTMI_MIP_HDR_*) ----
// A texel is a uint2 of four halfs; a sum starts from +0 and takes its taps in index order, s = s + (w * v), the product and the sum
// rounded on their own (-ffp-contract=off), w = (float)q * 2^-14 and the half as a float both exact.  An entry between the two
// passes is the four sums, 16 bytes.  The kernels are the integer ones' templates with KIND = kRGBA16F: the kind chooses the texel,
// the number type and the finish under `if constexpr`, and the integer instances' code is what it was.
inline bool rangeFitsKind(int kind, uint32_t range) // exactly one flag with RGBA16F, none with any other kind
{
    return kind == kRGBA16F ? range == kHdrNonnegative || range == kHdrSigned : range == 0;
}

inline float hdrRangeLow(uint32_t range) // the lower clamp; the upper one is 65504 under both
{
    return range == kHdrSigned ? -65504.0f : 0.0f;
}

__device__ __forceinline__ float halfValue(uint32_t bits) // of the low 16 bits
{
    return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(bits)));
}

// the half of a second pass's sum: clamped to [lo, 65504] by comparisons (a NaN passes both), then round-to-nearest-even with
// subnormal halfs; a sum is never -0, a small negative one under lo = -65504 becomes 0x8000
__device__ __forceinline__ uint32_t rangedHalf(float s, float lo)
{
    const float c = s < lo ? lo : (s > 65504.0f ? 65504.0f : s);
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(c));
}

__device__ __forceinline__ uint2 rangedTexel(const float (&s)[4], float lo)
{
    return make_uint2(rangedHalf(s[0], lo) | (rangedHalf(s[1], lo) << 16), rangedHalf(s[2], lo) | (rangedHalf(s[3], lo) << 16));
}
} // namespace
