// TEST INFRASTRUCTURE ONLY: one client of cvtt::Kernels, compiled twice from this very source --
//   against the reference's header and sources (oracle/Makefile, target ref -> oracle/_ref/dropin_client_ref), and
//   against include/cvtt/ConvectionKernels.h and libcvtt_mi355x.so (tests/test_dropin_differential.py).
// Both programs run on the same box and must print the same lines (the reference reads the host's RCPPS, and so does
// cvttmi_create).  Nothing of the project's C ABI is used here; our header is told apart by its include guard, and that
// guard gates only the *Batch calls (the reference build loops over the one-group entry and prints the same keys).
//
//   dropin_client <section> [repetitions]
//   sections: host s3tc bc7 bc6h etc eac decode batch threads
// Every line: <section> <entry> <option set> <group> <hex or number>.  The first line is the SHA-256 of this file as the
// build passed it in (-DCLIENT_SRC_SHA=...), so that a stale binary is recognised instead of compared.
//
// Content comes from an integer generator (SplitMix64); no floating point goes into it.
#include "ConvectionKernels.h"

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#ifndef CLIENT_SRC_SHA
#define CLIENT_SRC_SHA unknown
#endif
#define STR2(x) #x
#define STR(x) STR2(x)

namespace K = cvtt::Kernels;
static const unsigned G8 = cvtt::NumParallelBlocks;

// ---------------------------------------------------------------- generator
struct Rng
{
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(((next() >> 32) * (uint64_t)n) >> 32); }
    int range(int lo, int hi) { return lo + (int)below((uint32_t)(hi - lo + 1)); } // inclusive
};

// ---------------------------------------------------------------- content
// One generic block of 16 pixels x 4 channels of integers in [lo, hi]; the pixel types are made from it.
// kinds: 0 noise, 1 smooth gradient, 2 two colours split inside the block, 3 solid, 4 narrow range, 5 extremes,
//        6 (group level only) the kinds mixed block by block, 7 alpha at 0, around the middle and near the top.
// low: base colours come from the lower half of the range (the signed types get their negative values from it).
enum { kNoise, kGradient, kTwo, kSolid, kNarrow, kExtremes, kMixed, kAlpha, kNumGroups };
static const char *const kGroupNames[kNumGroups] = {"noise", "gradient", "two", "solid", "narrow", "extremes", "mixed", "alpha"};

struct IntBlock { int v[16][4]; };

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static void genBlock(IntBlock &b, int kind, Rng &rng, int lo, int hi, bool low)
{
    const int span = hi - lo;
    const int baseHi = low ? lo + span / 2 - 1 : hi;
    switch (kind)
    {
    default:
    case kNoise:
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                b.v[p][c] = rng.range(lo, hi);
        if (low)
            for (int c = 0; c < 4; c++)
            {
                const uint32_t p = rng.below(16); // (a statement of its own: the order of two calls in one expression is the compiler's)
                b.v[p][c] = rng.range(lo, baseHi);
            }
        break;
    case kGradient:
    {
        int c0[4], dx[4], dy[4];
        const int step = span / 20 > 0 ? span / 20 : 1;
        for (int c = 0; c < 4; c++)
        {
            c0[c] = rng.range(lo, baseHi);
            dx[c] = rng.range(-step, step);
            dy[c] = rng.range(-step, step);
        }
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                b.v[p][c] = clampi(c0[c] + (p & 3) * dx[c] + (p >> 2) * dy[c], lo, hi);
        break;
    }
    case kTwo:
    {
        int a[4], z[4];
        for (int c = 0; c < 4; c++)
        {
            a[c] = rng.range(lo, baseHi);
            z[c] = rng.range(lo, hi);
        }
        const uint32_t mask = (rng.below(1u << 16) | 0x8000u) & ~1u; // both colours present
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                b.v[p][c] = ((mask >> p) & 1) ? z[c] : a[c];
        break;
    }
    case kSolid:
    {
        int a[4];
        for (int c = 0; c < 4; c++)
            a[c] = rng.range(lo, baseHi);
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                b.v[p][c] = a[c];
        break;
    }
    case kNarrow:
    {
        int a[4];
        for (int c = 0; c < 4; c++)
            a[c] = rng.range(lo, baseHi - 3);
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                b.v[p][c] = a[c] + (int)rng.below(4);
        break;
    }
    case kExtremes:
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                b.v[p][c] = rng.below(2) ? hi : lo;
        for (int c = 0; c < 4; c++)
        {
            b.v[0][c] = lo;
            b.v[1][c] = hi;
        }
        break;
    case kAlpha:
    {
        // alpha at 0, around the middle (127 / 128 of 255) and near the top (250 / 251 of 255), scaled to the range
        const int mid = lo + span / 2, top = hi - (span * 5) / 255;
        const int alphas[8] = {lo, mid - 1, mid, mid + 1, top, top + 1, hi, lo};
        for (int p = 0; p < 16; p++)
        {
            for (int c = 0; c < 3; c++)
                b.v[p][c] = rng.range(lo, hi);
            b.v[p][3] = alphas[rng.below(8)];
        }
        for (int c = 0; c < 3; c++)
            b.v[0][c] = rng.range(lo, baseHi);
        b.v[0][3] = lo;
        break;
    }
    }
}

static int kindOfBlock(int group, unsigned block)
{
    static const int mixed[8] = {kNoise, kGradient, kTwo, kSolid, kNarrow, kExtremes, kAlpha, kNoise};
    return group == kMixed ? mixed[block % 8] : group;
}

static void genGroup(IntBlock *blocks, int group, uint64_t seed, int lo, int hi, bool low)
{
    Rng rng(seed * 1000003ULL + (uint64_t)group * 7919ULL + 17);
    for (unsigned b = 0; b < G8; b++)
        genBlock(blocks[b], kindOfBlock(group, b), rng, lo, hi, low);
}

static void groupU8(cvtt::PixelBlockU8 *out, int group, uint64_t seed = 1)
{
    IntBlock ib[8];
    genGroup(ib, group, seed, 0, 255, false);
    for (unsigned b = 0; b < G8; b++)
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                out[b].m_pixels[p][c] = (uint8_t)ib[b].v[p][c];
}

static void groupS8(cvtt::PixelBlockS8 *out, int group)
{
    IntBlock ib[8];
    genGroup(ib, group, 2, -128, 127, true);
    for (unsigned b = 0; b < G8; b++)
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
                out[b].m_pixels[p][c] = (int8_t)ib[b].v[p][c];
}

// R11: the unsigned form clamps to 0..2047, the signed one to -1023..1023 (stored 1..2047); the extremes group sits at and
// beyond both clamps
static void groupR11(cvtt::PixelBlockScalarS16 *out, int group, bool isSigned)
{
    IntBlock ib[8];
    const int lo = isSigned ? -1023 : 0, hi = isSigned ? 1023 : 2047;
    genGroup(ib, group, isSigned ? 4 : 3, lo, hi, isSigned);
    static const int beyondU[8] = {-1, 0, 2047, 2048, -32768, 32767, 1, 2046};
    static const int beyondS[8] = {-1024, -1023, 1023, 1024, -32768, 32767, -1022, 1022};
    Rng rng(99 + (uint64_t)group + (isSigned ? 1000 : 0));
    for (unsigned b = 0; b < G8; b++)
        for (int p = 0; p < 16; p++)
        {
            int v = ib[b].v[p][0];
            if (kindOfBlock(group, b) == kExtremes)
                v = (isSigned ? beyondS : beyondU)[p < 8 ? p : (int)rng.below(8)];
            out[b].m_pixels[p] = (int16_t)v;
        }
}

// half-float bit patterns, finite only (0 .. 0x7BFF); the signed form sets sign bits in every group
static void groupF16(cvtt::PixelBlockF16 *out, int group, bool isSigned)
{
    IntBlock ib[8];
    // bit patterns are monotonic in value, so gradients, narrow ranges and two-colour splits can be made in bit space
    const bool wide = group == kNoise || group == kExtremes;
    genGroup(ib, group, isSigned ? 6 : 5, wide ? 0 : 0x2C00, wide ? 0x7BFF : 0x4FFF, false);
    static const int extremes[6] = {0x0000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0x3C00};
    Rng rng(77 + (uint64_t)group + (isSigned ? 1000 : 0));
    for (unsigned b = 0; b < G8; b++)
    {
        const int kind = kindOfBlock(group, b);
        // sign: per pixel and channel for noise / extremes / alpha, per block and channel otherwise (a solid block stays solid)
        const uint32_t blockSigns = rng.below(16) | 1u;
        for (int p = 0; p < 16; p++)
            for (int c = 0; c < 4; c++)
            {
                int bits = ib[b].v[p][c];
                if (kind == kExtremes)
                    bits = extremes[rng.below(6)];
                if (isSigned)
                {
                    const bool perPixel = kind == kNoise || kind == kExtremes || kind == kAlpha;
                    const bool neg = perPixel ? (rng.below(2) != 0 || p == 0) : ((blockSigns >> c) & 1) != 0;
                    if (neg && bits != 0)
                        bits |= 0x8000;
                }
                if (c == 3)
                    bits = 0x3C00;
                out[b].m_pixels[p][c] = (int16_t)(uint16_t)bits;
            }
        if (isSigned && kind == kExtremes)
            out[b].m_pixels[0][0] = (int16_t)(uint16_t)0xFBFF;
    }
}

// the U / S wrappers can only be told apart on content with negative values: checked here, for every group
static int contentSelfCheck()
{
    int bad = 0;
    for (int g = 0; g < kNumGroups; g++)
    {
        cvtt::PixelBlockS8 s8[8];
        cvtt::PixelBlockScalarS16 r11[8];
        cvtt::PixelBlockF16 f16[8];
        groupS8(s8, g);
        groupR11(r11, g, true);
        groupF16(f16, g, true);
        int neg0 = 0, neg1 = 0, negR = 0, negH = 0;
        for (unsigned b = 0; b < G8; b++)
            for (int p = 0; p < 16; p++)
            {
                neg0 += s8[b].m_pixels[p][0] < 0;
                neg1 += s8[b].m_pixels[p][1] < 0;
                negR += r11[b].m_pixels[p] < 0;
                for (int c = 0; c < 3; c++)
                    negH += f16[b].m_pixels[p][c] < 0;
            }
        if (!neg0 || !neg1 || !negR || !negH)
        {
            fprintf(stderr, "content: group %s has no negative value (s8 %d %d, r11 %d, f16 %d)\n", kGroupNames[g], neg0, neg1, negR, negH);
            bad++;
        }
    }
    return bad;
}

// ---------------------------------------------------------------- options and plans
enum { kNumOptionSets = 6 };
static const char *const kOptionNames[kNumOptionSets] = {"default", "fastest", "ultra_pt", "uniform_w", "s3tc_ex709", "sp2_rr1"};
static cvtt::Options optionSet(int i)
{
    cvtt::Options o;
    switch (i)
    {
    case 1:
        o.flags = cvtt::Flags::Fastest;
        break;
    case 2:
        o.flags = cvtt::Flags::Ultra | cvtt::Flags::BC7_RespectPunchThrough;
        o.threshold = 0.25f;
        break;
    case 3:
        o.flags = cvtt::Flags::Uniform;
        o.redWeight = 0.3f;
        o.greenWeight = 1.0f;
        o.blueWeight = 0.1f;
        o.alphaWeight = 2.0f;
        break;
    case 4:
        o.flags = cvtt::Flags::S3TC_Paranoid | cvtt::Flags::S3TC_Exhaustive | cvtt::Flags::ETC_UseFakeBT709;
        o.refineRoundsS3TC = 3;
        o.refineRoundsIIC = 3;
        break;
    case 5:
        o.seedPoints = 2;
        o.refineRoundsBC7 = 1;
        o.refineRoundsBC6H = 1;
        break;
    default:
        break;
    }
    return o;
}

// the Options the "differently allocated" ETC scratch is made under
static cvtt::Options otherAllocOptions()
{
    cvtt::Options o;
    o.redWeight = 0.9f;
    o.greenWeight = 0.3f;
    o.blueWeight = 0.6f;
    return o;
}

static void fineTuningSet(cvtt::BC7FineTuningParams &ft, int i)
{
    static const uint32_t density[4] = {5, 30, 70, 100};
    Rng rng(4242 + (uint64_t)i);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(&ft);
    for (size_t k = 0; k < sizeof(ft); k++)
        bytes[k] = rng.below(100) < density[i & 3] ? (uint8_t)(1 + rng.below(4)) : (uint8_t)0;
}

enum { kNumPlans = 5 };
static const char *const kPlanNames[kNumPlans] = {"plan_default", "plan_q1", "plan_q20", "plan_q90", "plan_ft"};
static void planSet(cvtt::BC7EncodingPlan &plan, int i)
{
    switch (i)
    {
    case 1: K::ConfigureBC7EncodingPlanFromQuality(plan, 1); break;
    case 2: K::ConfigureBC7EncodingPlanFromQuality(plan, 20); break;
    case 3: K::ConfigureBC7EncodingPlanFromQuality(plan, 90); break;
    case 4:
    {
        cvtt::BC7FineTuningParams ft;
        fineTuningSet(ft, 2);
        K::ConfigureBC7EncodingPlanFromFineTuningParams(plan, ft);
        break;
    }
    default: break;
    }
}

// ---------------------------------------------------------------- output
static void emitHex(const char *section, const char *entry, const char *opt, const char *group, const void *p, size_t n)
{
    static const char digits[] = "0123456789abcdef";
    std::string s;
    s.reserve(2 * n);
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; i++)
    {
        s += digits[b[i] >> 4];
        s += digits[b[i] & 15];
    }
    printf("%s %s %s %s %s\n", section, entry, opt, group, s.c_str());
}
static void emitNum(const char *section, const char *entry, const char *opt, const char *group, long long v)
{
    printf("%s %s %s %s %lld\n", section, entry, opt, group, v);
}

// ---------------------------------------------------------------- scratch allocator with a ledger
// The client's free function must see the pointer, the size and the context it handed out.  The contexts are the
// addresses of Ledger objects, but they are only compared, never followed: a Release* that passes something else is counted.
struct Ledger
{
    int unused;
    Ledger() : unused(0) {}
};
struct LedgerEntry { void *p; size_t size; void *context; };
static std::mutex g_ledgerMutex;
static std::vector<LedgerEntry> g_ledgerLive;
static int g_releaseMismatches = 0;
static void *ledgerAlloc(void *context, size_t size)
{
    void *p = NULL;
    if (posix_memalign(&p, 64, size ? size : 1) != 0)
        return NULL;
    const LedgerEntry e = {p, size, context};
    std::lock_guard<std::mutex> lock(g_ledgerMutex);
    g_ledgerLive.push_back(e);
    return p;
}
static void ledgerFree(void *context, void *ptr, size_t size)
{
    std::lock_guard<std::mutex> lock(g_ledgerMutex);
    for (size_t i = 0; i < g_ledgerLive.size(); i++)
        if (g_ledgerLive[i].p == ptr)
        {
            if (g_ledgerLive[i].size != size || g_ledgerLive[i].context != context)
                g_releaseMismatches++;
            g_ledgerLive.erase(g_ledgerLive.begin() + (long)i);
            free(ptr);
            return;
        }
    g_releaseMismatches++; // not a pointer that is out
}
static int ledgerMismatches()
{
    std::lock_guard<std::mutex> lock(g_ledgerMutex);
    return g_releaseMismatches;
}
static int ledgerLive()
{
    std::lock_guard<std::mutex> lock(g_ledgerMutex);
    return (int)g_ledgerLive.size();
}

// ---------------------------------------------------------------- host section
typedef void (*EncodeU8Fn)(uint8_t *, const cvtt::PixelBlockU8 *, const cvtt::Options &);
typedef void (*EncodeS8Fn)(uint8_t *, const cvtt::PixelBlockS8 *, const cvtt::Options &);
typedef void (*EncodeF16Fn)(uint8_t *, const cvtt::PixelBlockF16 *, const cvtt::Options &);
typedef void (*EncodeBC7Fn)(uint8_t *, const cvtt::PixelBlockU8 *, const cvtt::Options &, const cvtt::BC7EncodingPlan &);
typedef void (*EncodeETC1Fn)(uint8_t *, const cvtt::PixelBlockU8 *, const cvtt::Options &, cvtt::ETC1CompressionData *);
typedef void (*EncodeETC2Fn)(uint8_t *, const cvtt::PixelBlockU8 *, const cvtt::Options &, cvtt::ETC2CompressionData *);
typedef void (*EncodeR11Fn)(uint8_t *, const cvtt::PixelBlockScalarS16 *, bool, const cvtt::Options &);
typedef void (*DecodeU8Fn)(cvtt::PixelBlockU8 *, const uint8_t *);
typedef void (*DecodeF16Fn)(cvtt::PixelBlockF16 *, const uint8_t *);
typedef void (*PlanQualityFn)(cvtt::BC7EncodingPlan &, int);
typedef bool (*PlanFineFn)(cvtt::BC7EncodingPlan &, const cvtt::BC7FineTuningParams &);
typedef cvtt::ETC2CompressionData *(*Alloc2Fn)(K::allocFunc_t, void *, const cvtt::Options &);
typedef void (*Release2Fn)(cvtt::ETC2CompressionData *, K::freeFunc_t);
typedef cvtt::ETC1CompressionData *(*Alloc1Fn)(K::allocFunc_t, void *);
typedef void (*Release1Fn)(cvtt::ETC1CompressionData *, K::freeFunc_t);
typedef void *(*AllocCallbackFn)(void *, size_t);
typedef void (*FreeCallbackFn)(void *, void *, size_t);

// Every entry point assigned to a pointer of exactly the type the reference declares: a drifted signature does not compile.
static const EncodeU8Fn kEncodeU8[] = {&K::EncodeBC1, &K::EncodeBC2, &K::EncodeBC3, &K::EncodeBC4U, &K::EncodeBC5U, &K::EncodeETC2Alpha};
static const char *const kEncodeU8Names[] = {"EncodeBC1", "EncodeBC2", "EncodeBC3", "EncodeBC4U", "EncodeBC5U", "EncodeETC2Alpha"};
static const size_t kEncodeU8Bytes[] = {8, 16, 16, 8, 16, 8};
static const EncodeS8Fn kEncodeS8[] = {&K::EncodeBC4S, &K::EncodeBC5S};
static const char *const kEncodeS8Names[] = {"EncodeBC4S", "EncodeBC5S"};
static const size_t kEncodeS8Bytes[] = {8, 16};
static const EncodeF16Fn kEncodeF16[] = {&K::EncodeBC6HU, &K::EncodeBC6HS};
static const char *const kEncodeF16Names[] = {"EncodeBC6HU", "EncodeBC6HS"};
static const EncodeBC7Fn kEncodeBC7 = &K::EncodeBC7;
static const EncodeETC1Fn kEncodeETC1 = &K::EncodeETC1;
static const EncodeETC2Fn kEncodeETC2[] = {&K::EncodeETC2, &K::EncodeETC2RGBA, &K::EncodeETC2PunchthroughAlpha};
static const char *const kEncodeETC2Names[] = {"EncodeETC2", "EncodeETC2RGBA", "EncodeETC2PunchthroughAlpha"};
static const size_t kEncodeETC2Bytes[] = {8, 16, 8};
static const EncodeR11Fn kEncodeR11 = &K::EncodeETC2Alpha11;
static const DecodeU8Fn kDecodeBC7 = &K::DecodeBC7;
static const DecodeF16Fn kDecodeF16[] = {&K::DecodeBC6HU, &K::DecodeBC6HS};
static const PlanQualityFn kPlanQuality = &K::ConfigureBC7EncodingPlanFromQuality;
static const PlanFineFn kPlanFine = &K::ConfigureBC7EncodingPlanFromFineTuningParams;
static const Alloc2Fn kAlloc2 = &K::AllocETC2Data;
static const Release2Fn kRelease2 = &K::ReleaseETC2Data;
static const Alloc1Fn kAlloc1 = &K::AllocETC1Data;
static const Release1Fn kRelease1 = &K::ReleaseETC1Data;
static K::allocFunc_t *const kAllocCallback = static_cast<AllocCallbackFn>(&ledgerAlloc);
static K::freeFunc_t *const kFreeCallback = static_cast<FreeCallbackFn>(&ledgerFree);

template<class T, size_t N> static size_t countOf(const T (&)[N]) { return N; }

// the plan has padding after mode0PartitionEnabled and at its end: its bytes are printed field by field at the fields' own
// offsets over zeros, which shows the layout and leaves the padding out
#define PLAN_FIELD(f) memcpy(bytes + offsetof(cvtt::BC7EncodingPlan, f), &plan.f, sizeof(plan.f))
static void emitPlan(const char *section, const char *entry, const char *opt, const char *group, const cvtt::BC7EncodingPlan &plan)
{
    uint8_t bytes[sizeof(cvtt::BC7EncodingPlan)];
    memset(bytes, 0, sizeof(bytes));
    PLAN_FIELD(mode1PartitionEnabled);
    PLAN_FIELD(mode2PartitionEnabled);
    PLAN_FIELD(mode3PartitionEnabled);
    PLAN_FIELD(mode0PartitionEnabled);
    PLAN_FIELD(mode7RGBAPartitionEnabled);
    PLAN_FIELD(mode7RGBPartitionEnabled);
    PLAN_FIELD(mode4SP);
    PLAN_FIELD(mode5SP);
    bytes[offsetof(cvtt::BC7EncodingPlan, mode6Enabled)] = plan.mode6Enabled ? 1 : 0;
    PLAN_FIELD(seedPointsForShapeRGB);
    PLAN_FIELD(seedPointsForShapeRGBA);
    PLAN_FIELD(rgbaShapeList);
    PLAN_FIELD(rgbaNumShapesToEvaluate);
    PLAN_FIELD(rgbShapeList);
    PLAN_FIELD(rgbNumShapesToEvaluate);
    emitHex(section, entry, opt, group, bytes, sizeof(bytes));
}

// both builds must feed the encoders the same inputs: a digest (FNV-1a) of every generated group, per pixel type
static unsigned long long fnv(unsigned long long h, const void *p, size_t n)
{
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; i++)
        h = (h ^ b[i]) * 0x100000001B3ULL;
    return h;
}
static void emitContentDigests()
{
    unsigned long long h[7];
    for (int i = 0; i < 7; i++)
        h[i] = 0xCBF29CE484222325ULL;
    for (int g = 0; g < kNumGroups; g++)
    {
        cvtt::PixelBlockU8 u8[8];
        cvtt::PixelBlockS8 s8[8];
        cvtt::PixelBlockF16 f16[8];
        cvtt::PixelBlockScalarS16 r11[8];
        groupU8(u8, g);
        h[0] = fnv(h[0], u8, sizeof(u8));
        groupS8(s8, g);
        h[1] = fnv(h[1], s8, sizeof(s8));
        for (int s = 0; s < 2; s++)
        {
            groupF16(f16, g, s != 0);
            h[2 + s] = fnv(h[2 + s], f16, sizeof(f16));
            groupR11(r11, g, s != 0);
            h[4 + s] = fnv(h[4 + s], r11, sizeof(r11));
        }
    }
    for (int t = 0; t < 16; t++)
    {
        cvtt::PixelBlockU8 u8[8];
        groupU8(u8, kNoise, 100 + (uint64_t)t);
        h[6] = fnv(h[6], u8, sizeof(u8));
    }
    static const char *const names[7] = {"PixelBlockU8", "PixelBlockS8", "PixelBlockF16/unsigned", "PixelBlockF16/signed",
                                         "PixelBlockScalarS16/unsigned", "PixelBlockScalarS16/signed", "PixelBlockU8/threads"};
    for (int i = 0; i < 7; i++)
        printf("host content - %s %016llx\n", names[i], h[i]);
}

static int sectionHost()
{
    emitContentDigests();
    const size_t entries = countOf(kEncodeU8) + countOf(kEncodeS8) + countOf(kEncodeF16) + countOf(kEncodeETC2) + countOf(kDecodeF16) +
                           (kEncodeBC7 != NULL) + (kEncodeETC1 != NULL) + (kEncodeR11 != NULL) + (kDecodeBC7 != NULL) + (kPlanQuality != NULL) + (kPlanFine != NULL) +
                           (kAlloc2 != NULL) + (kRelease2 != NULL) + (kAlloc1 != NULL) + (kRelease1 != NULL);
    emitNum("host", "signatures", "-", "entries", (long long)entries);
    emitNum("host", "signatures", "-", "callbacks", (kAllocCallback != NULL) + (kFreeCallback != NULL));

    emitNum("host", "sizeof", "-", "Options", sizeof(cvtt::Options));
    emitNum("host", "sizeof", "-", "BC7EncodingPlan", sizeof(cvtt::BC7EncodingPlan));
    emitNum("host", "sizeof", "-", "BC7FineTuningParams", sizeof(cvtt::BC7FineTuningParams));
    emitNum("host", "sizeof", "-", "PixelBlockU8", sizeof(cvtt::PixelBlockU8));
    emitNum("host", "sizeof", "-", "PixelBlockS8", sizeof(cvtt::PixelBlockS8));
    emitNum("host", "sizeof", "-", "PixelBlockScalarS16", sizeof(cvtt::PixelBlockScalarS16));
    emitNum("host", "sizeof", "-", "PixelBlockF16", sizeof(cvtt::PixelBlockF16));
    emitNum("host", "constant", "-", "NumParallelBlocks", cvtt::NumParallelBlocks);
    emitNum("host", "constant", "-", "kNumRGBAShapes", cvtt::BC7EncodingPlan::kNumRGBAShapes);
    emitNum("host", "constant", "-", "kNumRGBShapes", cvtt::BC7EncodingPlan::kNumRGBShapes);

    {
        cvtt::Options o; // 11 four-byte fields, no padding
        emitHex("host", "default", "-", "Options", &o, sizeof(o));
        cvtt::BC7FineTuningParams ft; // bytes only, no padding
        emitHex("host", "default", "-", "BC7FineTuningParams", &ft, sizeof(ft));
        cvtt::BC7EncodingPlan plan;
        emitPlan("host", "default", "-", "BC7EncodingPlan", plan);
        for (int i = 0; i < kNumOptionSets; i++)
        {
            o = optionSet(i);
            emitHex("host", "options", kOptionNames[i], "Options", &o, sizeof(o));
        }
    }
#define FLAG(name) do { const uint32_t v = cvtt::Flags::name; printf("host flag - %s %08x\n", #name, (unsigned)v); } while (0)
    FLAG(BC7_FastIndexing);
    FLAG(BC7_TrySingleColor);
    FLAG(BC7_RespectPunchThrough);
    FLAG(BC6H_FastIndexing);
    FLAG(S3TC_Exhaustive);
    FLAG(S3TC_Paranoid);
    FLAG(Uniform);
    FLAG(ETC_UseFakeBT709);
    FLAG(ETC_FakeBT709Accurate);
    FLAG(Fastest);
    FLAG(Faster);
    FLAG(Fast);
    FLAG(Default);
    FLAG(Better);
    FLAG(Ultra);
#undef FLAG
    static const int qualities[] = {-5, 0, 1, 2, 17, 50, 99, 100, 101, 1000};
    for (size_t i = 0; i < countOf(qualities); i++)
    {
        cvtt::BC7EncodingPlan plan;
        kPlanQuality(plan, qualities[i]);
        char name[32];
        snprintf(name, sizeof(name), "q%d", qualities[i]);
        emitPlan("host", "plan_from_quality", "-", name, plan);
    }
    for (int i = 0; i < 4; i++)
    {
        cvtt::BC7FineTuningParams ft;
        fineTuningSet(ft, i);
        cvtt::BC7EncodingPlan plan;
        const bool ok = kPlanFine(plan, ft);
        char name[32];
        snprintf(name, sizeof(name), "ft%d", i);
        emitHex("host", "fine_tuning_params", "-", name, &ft, sizeof(ft));
        emitNum("host", "plan_from_fine_tuning_returns", "-", name, ok ? 1 : 0);
        emitPlan("host", "plan_from_fine_tuning", "-", name, plan);
    }
    return 0;
}

// ---------------------------------------------------------------- encode sections
static int sectionS3TC()
{
    for (int o = 0; o < kNumOptionSets; o++)
    {
        const cvtt::Options options = optionSet(o);
        for (int g = 0; g < kNumGroups; g++)
        {
            cvtt::PixelBlockU8 u8[8];
            cvtt::PixelBlockS8 s8[8];
            groupU8(u8, g);
            groupS8(s8, g);
            uint8_t out[128];
            for (size_t e = 0; e < 5; e++) // (EncodeETC2Alpha, the table's last entry, belongs to the eac section)
            {
                memset(out, 0xEE, sizeof(out));
                kEncodeU8[e](out, u8, options);
                emitHex("s3tc", kEncodeU8Names[e], kOptionNames[o], kGroupNames[g], out, kEncodeU8Bytes[e] * G8);
            }
            for (size_t e = 0; e < countOf(kEncodeS8); e++)
            {
                memset(out, 0xEE, sizeof(out));
                kEncodeS8[e](out, s8, options);
                emitHex("s3tc", kEncodeS8Names[e], kOptionNames[o], kGroupNames[g], out, kEncodeS8Bytes[e] * G8);
            }
        }
    }
    return 0;
}

static int sectionBC7()
{
    uint8_t out[128];
    cvtt::BC7EncodingPlan defaultPlan;
    for (int o = 0; o < kNumOptionSets; o++)
    {
        const cvtt::Options options = optionSet(o);
        for (int g = 0; g < kNumGroups; g++)
        {
            cvtt::PixelBlockU8 u8[8];
            groupU8(u8, g);
            memset(out, 0xEE, sizeof(out));
            K::EncodeBC7(out, u8, options, defaultPlan);
            emitHex("bc7", "EncodeBC7", kOptionNames[o], kGroupNames[g], out, sizeof(out));
        }
    }
    static const int planOptionSets[2] = {0, 2}; // default and punch-through
    for (int pi = 1; pi < kNumPlans; pi++) // (the default plan ran above)
    {
        cvtt::BC7EncodingPlan plan;
        planSet(plan, pi);
        for (int k = 0; k < 2; k++)
        {
            const cvtt::Options options = optionSet(planOptionSets[k]);
            const std::string name = std::string(kOptionNames[planOptionSets[k]]) + "/" + kPlanNames[pi];
            for (int g = 0; g < kNumGroups; g++)
            {
                cvtt::PixelBlockU8 u8[8];
                groupU8(u8, g);
                memset(out, 0xEE, sizeof(out));
                K::EncodeBC7(out, u8, options, plan);
                emitHex("bc7", "EncodeBC7", name.c_str(), kGroupNames[g], out, sizeof(out));
            }
        }
    }
    return 0;
}

static int sectionBC6H()
{
    uint8_t out[128];
    for (int o = 0; o < kNumOptionSets; o++)
    {
        const cvtt::Options options = optionSet(o);
        for (int g = 0; g < kNumGroups; g++)
            for (size_t e = 0; e < countOf(kEncodeF16); e++)
            {
                cvtt::PixelBlockF16 f16[8];
                groupF16(f16, g, e == 1);
                memset(out, 0xEE, sizeof(out));
                kEncodeF16[e](out, f16, options);
                emitHex("bc6h", kEncodeF16Names[e], kOptionNames[o], kGroupNames[g], out, sizeof(out));
            }
    }
    return 0;
}

static int sectionETC()
{
    Ledger ledger;
    int nullAllocs = 0;
    for (int o = 0; o < kNumOptionSets; o++)
    {
        const cvtt::Options options = optionSet(o);
        for (int scratch = 0; scratch < 2; scratch++) // 0: allocated under the call's own Options, 1: under other weights
        {
            const std::string name = std::string(kOptionNames[o]) + (scratch ? "/other_alloc" : "/own_alloc");
            const cvtt::Options allocOptions = scratch ? otherAllocOptions() : options;
            for (int g = 0; g < kNumGroups; g++)
            {
                cvtt::PixelBlockU8 u8[8];
                groupU8(u8, g);
                uint8_t out[128];
                cvtt::ETC1CompressionData *data1 = K::AllocETC1Data(ledgerAlloc, &ledger);
                nullAllocs += data1 == NULL;
                if (scratch == 0 && data1)
                {
                    memset(out, 0xEE, sizeof(out));
                    K::EncodeETC1(out, u8, options, data1);
                    emitHex("etc", "EncodeETC1", name.c_str(), kGroupNames[g], out, 8 * G8);
                }
                if (data1)
                    K::ReleaseETC1Data(data1, ledgerFree);
                cvtt::ETC2CompressionData *data2 = K::AllocETC2Data(ledgerAlloc, &ledger, allocOptions);
                nullAllocs += data2 == NULL;
                if (!data2)
                    continue;
                for (size_t e = 0; e < countOf(kEncodeETC2); e++)
                {
                    memset(out, 0xEE, sizeof(out));
                    kEncodeETC2[e](out, u8, options, data2);
                    emitHex("etc", kEncodeETC2Names[e], name.c_str(), kGroupNames[g], out, kEncodeETC2Bytes[e] * G8);
                }
                K::ReleaseETC2Data(data2, ledgerFree);
            }
        }
    }
    emitNum("etc", "Alloc", "-", "null_results", nullAllocs);
    emitNum("etc", "Release", "-", "mismatches", ledgerMismatches());
    emitNum("etc", "Release", "-", "still_live", ledgerLive());
    return 0;
}

static int sectionEAC()
{
    uint8_t out[64];
    for (int o = 0; o < kNumOptionSets; o++)
    {
        const cvtt::Options options = optionSet(o);
        for (int g = 0; g < kNumGroups; g++)
        {
            cvtt::PixelBlockU8 u8[8];
            groupU8(u8, g);
            memset(out, 0xEE, sizeof(out));
            K::EncodeETC2Alpha(out, u8, options);
            emitHex("eac", "EncodeETC2Alpha", kOptionNames[o], kGroupNames[g], out, sizeof(out));
            for (int isSigned = 0; isSigned < 2; isSigned++)
            {
                cvtt::PixelBlockScalarS16 r11[8];
                groupR11(r11, g, isSigned != 0);
                memset(out, 0xEE, sizeof(out));
                kEncodeR11(out, r11, isSigned != 0, options);
                emitHex("eac", isSigned ? "EncodeETC2Alpha11/signed" : "EncodeETC2Alpha11/unsigned", kOptionNames[o], kGroupNames[g], out, sizeof(out));
            }
        }
    }
    return 0;
}

// ---------------------------------------------------------------- decode section
static void forcedBlocks(uint8_t *bytes, size_t numBlocks, bool bc7)
{
    Rng rng(bc7 ? 7007 : 6006);
    for (size_t i = 0; i < numBlocks; i++)
    {
        uint8_t *b = bytes + 16 * i;
        for (int k = 0; k < 16; k++)
            b[k] = (uint8_t)rng.below(256);
        if (bc7)
        {
            const unsigned m = (unsigned)(i % 9); // modes 0..7 by their unary prefix; 8 = the reserved all-zero mode byte
            b[0] = m < 8 ? (uint8_t)((b[0] & ~((2u << m) - 1u)) | (1u << m)) : (uint8_t)0;
        }
        else
            b[0] = (uint8_t)((b[0] & 0xE0) | (i % 32)); // each of the 32 five-bit headers
    }
}

static int sectionDecode()
{
    const cvtt::Options options;
    const cvtt::BC7EncodingPlan plan;
    for (int g = 0; g < kNumGroups; g++)
    {
        cvtt::PixelBlockU8 u8[8], back[8];
        cvtt::PixelBlockF16 f16[8], backF[8];
        uint8_t packed[128];
        groupU8(u8, g);
        K::EncodeBC7(packed, u8, options, plan);
        memset(back, 0xEE, sizeof(back));
        kDecodeBC7(back, packed);
        emitHex("decode", "DecodeBC7", "encoded", kGroupNames[g], back, sizeof(back));
        for (size_t e = 0; e < 2; e++)
        {
            groupF16(f16, g, e == 1);
            kEncodeF16[e](packed, f16, options);
            for (size_t d = 0; d < 2; d++) // either decoder on either encoder's blocks
            {
                memset(backF, 0xEE, sizeof(backF));
                kDecodeF16[d](backF, packed);
                const std::string name = std::string("encoded_by_") + kEncodeF16Names[e];
                emitHex("decode", d ? "DecodeBC6HS" : "DecodeBC6HU", name.c_str(), kGroupNames[g], backF, sizeof(backF));
            }
        }
    }
    const size_t groups = 64;
    std::vector<uint8_t> bytes(groups * G8 * 16);
    forcedBlocks(bytes.data(), groups * G8, true);
    for (size_t g = 0; g < groups; g++)
    {
        cvtt::PixelBlockU8 back[8];
        memset(back, 0xEE, sizeof(back));
        kDecodeBC7(back, &bytes[g * G8 * 16]);
        char name[16];
        snprintf(name, sizeof(name), "g%02d", (int)g);
        emitHex("decode", "DecodeBC7", "forced_modes", name, back, sizeof(back));
    }
    forcedBlocks(bytes.data(), groups * G8, false);
    for (size_t g = 0; g < groups; g++)
        for (size_t d = 0; d < 2; d++)
        {
            cvtt::PixelBlockF16 backF[8];
            memset(backF, 0xEE, sizeof(backF));
            kDecodeF16[d](backF, &bytes[g * G8 * 16]);
            char name[16];
            snprintf(name, sizeof(name), "g%02d", (int)g);
            emitHex("decode", d ? "DecodeBC6HS" : "DecodeBC6HU", "forced_headers", name, backF, sizeof(backF));
        }
    return 0;
}

// ---------------------------------------------------------------- batch section
// Every *Batch entry on 5 groups (40 blocks) at once; against the reference the same keys come from a loop over the one-group
// entry: batch = one-group loop = reference.
#ifdef CVTT_MI355X_CONVECTION_KERNELS_H
#define BATCH_OR_LOOP(batchCall, loopCall) do { batchCall; } while (0)
#else
#define BATCH_OR_LOOP(batchCall, loopCall) do { for (size_t g = 0; g < kBatchGroups; g++) { loopCall; } } while (0)
#endif
static const size_t kBatchGroups = 5;
static const size_t kBatchBlocks = kBatchGroups * 8;

static void emitBatch(const char *entry, const char *opt, const uint8_t *out, size_t bytesPerGroup)
{
    for (size_t g = 0; g < kBatchGroups; g++)
        emitHex("batch", entry, opt, kGroupNames[g], out + g * bytesPerGroup, bytesPerGroup);
}

static int sectionBatch()
{
    static const int sets[2] = {0, 2};
    std::vector<cvtt::PixelBlockU8> u8(kBatchBlocks);
    std::vector<cvtt::PixelBlockS8> s8(kBatchBlocks);
    std::vector<cvtt::PixelBlockF16> hu(kBatchBlocks), hs(kBatchBlocks);
    std::vector<cvtt::PixelBlockScalarS16> ru(kBatchBlocks), rs(kBatchBlocks);
    for (size_t g = 0; g < kBatchGroups; g++)
    {
        groupU8(&u8[g * 8], (int)g);
        groupS8(&s8[g * 8], (int)g);
        groupF16(&hu[g * 8], (int)g, false);
        groupF16(&hs[g * 8], (int)g, true);
        groupR11(&ru[g * 8], (int)g, false);
        groupR11(&rs[g * 8], (int)g, true);
    }
    std::vector<uint8_t> out(kBatchBlocks * 16), bc7(kBatchBlocks * 16), bc6u(kBatchBlocks * 16), bc6s(kBatchBlocks * 16);
    cvtt::BC7EncodingPlan plan;
    K::ConfigureBC7EncodingPlanFromQuality(plan, 20);
    Ledger ledger;
    for (int k = 0; k < 2; k++)
    {
        const cvtt::Options options = optionSet(sets[k]);
        const char *on = kOptionNames[sets[k]];
        uint8_t *o = out.data();
#define RUN(name, bytesPerBlock, batchCall, loopCall) \
        do { memset(o, 0xEE, out.size()); BATCH_OR_LOOP(batchCall, loopCall); emitBatch(name, on, o, (bytesPerBlock) * 8); } while (0)
        RUN("EncodeBC1", 8, K::EncodeBC1Batch(o, u8.data(), kBatchBlocks, options), K::EncodeBC1(o + g * 64, &u8[g * 8], options));
        RUN("EncodeBC2", 16, K::EncodeBC2Batch(o, u8.data(), kBatchBlocks, options), K::EncodeBC2(o + g * 128, &u8[g * 8], options));
        RUN("EncodeBC3", 16, K::EncodeBC3Batch(o, u8.data(), kBatchBlocks, options), K::EncodeBC3(o + g * 128, &u8[g * 8], options));
        RUN("EncodeBC4U", 8, K::EncodeBC4UBatch(o, u8.data(), kBatchBlocks, options), K::EncodeBC4U(o + g * 64, &u8[g * 8], options));
        RUN("EncodeBC4S", 8, K::EncodeBC4SBatch(o, s8.data(), kBatchBlocks, options), K::EncodeBC4S(o + g * 64, &s8[g * 8], options));
        RUN("EncodeBC5U", 16, K::EncodeBC5UBatch(o, u8.data(), kBatchBlocks, options), K::EncodeBC5U(o + g * 128, &u8[g * 8], options));
        RUN("EncodeBC5S", 16, K::EncodeBC5SBatch(o, s8.data(), kBatchBlocks, options), K::EncodeBC5S(o + g * 128, &s8[g * 8], options));
        RUN("EncodeBC6HU", 16, K::EncodeBC6HUBatch(o, hu.data(), kBatchBlocks, options), K::EncodeBC6HU(o + g * 128, &hu[g * 8], options));
        if (k == 0)
            bc6u = out;
        RUN("EncodeBC6HS", 16, K::EncodeBC6HSBatch(o, hs.data(), kBatchBlocks, options), K::EncodeBC6HS(o + g * 128, &hs[g * 8], options));
        if (k == 0)
            bc6s = out;
        RUN("EncodeBC7", 16, K::EncodeBC7Batch(o, u8.data(), kBatchBlocks, options, plan), K::EncodeBC7(o + g * 128, &u8[g * 8], options, plan));
        if (k == 0)
            bc7 = out;
        RUN("EncodeETC2Alpha", 8, K::EncodeETC2AlphaBatch(o, u8.data(), kBatchBlocks, options), K::EncodeETC2Alpha(o + g * 64, &u8[g * 8], options));
        RUN("EncodeETC2Alpha11/unsigned", 8, K::EncodeETC2Alpha11Batch(o, ru.data(), kBatchBlocks, false, options), K::EncodeETC2Alpha11(o + g * 64, &ru[g * 8], false, options));
        RUN("EncodeETC2Alpha11/signed", 8, K::EncodeETC2Alpha11Batch(o, rs.data(), kBatchBlocks, true, options), K::EncodeETC2Alpha11(o + g * 64, &rs[g * 8], true, options));
        // the ETC forms with scratch that was allocated under other weights than the call's
        cvtt::ETC1CompressionData *data1 = K::AllocETC1Data(ledgerAlloc, &ledger);
        cvtt::ETC2CompressionData *data2 = K::AllocETC2Data(ledgerAlloc, &ledger, otherAllocOptions());
        if (!data1 || !data2)
            return 4;
        RUN("EncodeETC1", 8, K::EncodeETC1Batch(o, u8.data(), kBatchBlocks, options), K::EncodeETC1(o + g * 64, &u8[g * 8], options, data1));
        RUN("EncodeETC2", 8, K::EncodeETC2Batch(o, u8.data(), kBatchBlocks, options, data2), K::EncodeETC2(o + g * 64, &u8[g * 8], options, data2));
        RUN("EncodeETC2RGBA", 16, K::EncodeETC2RGBABatch(o, u8.data(), kBatchBlocks, options, data2), K::EncodeETC2RGBA(o + g * 128, &u8[g * 8], options, data2));
        RUN("EncodeETC2PunchthroughAlpha", 8, K::EncodeETC2PunchthroughAlphaBatch(o, u8.data(), kBatchBlocks, options, data2),
            K::EncodeETC2PunchthroughAlpha(o + g * 64, &u8[g * 8], options, data2));
#undef RUN
        K::ReleaseETC2Data(data2, ledgerFree);
        K::ReleaseETC1Data(data1, ledgerFree);
    }
    // the decoders, on what the default set produced above
    {
        std::vector<cvtt::PixelBlockU8> back(kBatchBlocks);
        memset(back.data(), 0xEE, back.size() * sizeof(back[0]));
        BATCH_OR_LOOP(K::DecodeBC7Batch(back.data(), bc7.data(), kBatchBlocks), K::DecodeBC7(&back[g * 8], &bc7[g * 128]));
        emitBatch("DecodeBC7", "default", reinterpret_cast<const uint8_t *>(back.data()), 8 * sizeof(back[0]));
        std::vector<cvtt::PixelBlockF16> backF(kBatchBlocks);
        memset(backF.data(), 0xEE, backF.size() * sizeof(backF[0]));
        BATCH_OR_LOOP(K::DecodeBC6HUBatch(backF.data(), bc6u.data(), kBatchBlocks), K::DecodeBC6HU(&backF[g * 8], &bc6u[g * 128]));
        emitBatch("DecodeBC6HU", "default", reinterpret_cast<const uint8_t *>(backF.data()), 8 * sizeof(backF[0]));
        memset(backF.data(), 0xEE, backF.size() * sizeof(backF[0]));
        BATCH_OR_LOOP(K::DecodeBC6HSBatch(backF.data(), bc6s.data(), kBatchBlocks), K::DecodeBC6HS(&backF[g * 8], &bc6s[g * 128]));
        emitBatch("DecodeBC6HS", "default", reinterpret_cast<const uint8_t *>(backF.data()), 8 * sizeof(backF[0]));
    }
    emitNum("batch", "Release", "-", "mismatches", ledgerMismatches());
    emitNum("batch", "Release", "-", "still_live", ledgerLive());
    return 0;
}

// ---------------------------------------------------------------- threads section
// 16 caller threads, 13 kinds of call (the base and twelve that differ from it in exactly one thing): more kinds than the
// library's coalescer has slots, so calls that share a launch, calls on slots of their own and calls on the thread's own
// context all happen.  Each repetition is the kind's main call followed by EncodeBC1 with the same Options -- BC7 reads
// neither `threshold` nor `seedPoints`, BC1 reads both -- and must give the thread's first result again.
enum { kNumKinds = 13, kNumThreads = 16 };
static const char *const kKindNames[kNumKinds] = {"base", "flags_bit", "threshold", "red_weight", "green_weight", "blue_weight", "alpha_weight",
                                                  "refine_rounds_bc7", "seed_points", "plan_byte", "format_bc3", "etc2rgba_alloc_a", "etc2rgba_alloc_b"};
struct ThreadWork
{
    int kind;
    cvtt::PixelBlockU8 in[8];
    cvtt::Options options;
    cvtt::BC7EncodingPlan plan;
    uint8_t first[192], last[192];
    int differing;
    Ledger ledger;                  // (its address is the allocator context of this thread's scratch)
    cvtt::ETC2CompressionData *data; // every thread has its own
};

// the threads start every repetition together, so that calls of different kinds are in flight at the same time
struct Barrier
{
    std::atomic<int> arrived, generation;
    int parties;
    explicit Barrier(int n) : arrived(0), generation(0), parties(n) {}
    void wait()
    {
        const int g = generation.load();
        if (arrived.fetch_add(1) + 1 == parties)
        {
            arrived.store(0);
            generation.fetch_add(1);
        }
        else
            while (generation.load() == g)
                std::this_thread::yield();
    }
};

static void threadBody(ThreadWork *w, int repetitions, Barrier *barrier)
{
    for (int rep = 0; rep < repetitions; rep++)
    {
        uint8_t *dst = rep == 0 ? w->first : w->last;
        memset(dst, 0xEE, 192);
        barrier->wait();
        if (w->kind == 10)
            K::EncodeBC3(dst, w->in, w->options);
        else if (w->kind >= 11)
            K::EncodeETC2RGBA(dst, w->in, w->options, w->data);
        else
            K::EncodeBC7(dst, w->in, w->options, w->plan);
        K::EncodeBC1(dst + 128, w->in, w->options);
        if (rep > 0 && memcmp(w->first, w->last, 192) != 0)
            w->differing++;
    }
    if (repetitions == 1)
        memcpy(w->last, w->first, 192);
}

static int sectionThreads(int repetitions)
{
    if (repetitions < 1)
        repetitions = 1;
    static ThreadWork work[kNumThreads];
    for (int t = 0; t < kNumThreads; t++)
    {
        ThreadWork &w = work[t];
        w.kind = t < kNumKinds ? t : 0; // the base kind has four threads: the one the others would be mistaken for
        groupU8(w.in, kNoise, 100 + (uint64_t)t); // every thread its own input; noise has every alpha value
        w.differing = 0;
        w.data = NULL;
        if (w.kind >= 11)
        {
            w.data = K::AllocETC2Data(ledgerAlloc, &w.ledger, w.kind == 11 ? cvtt::Options() : otherAllocOptions());
            if (!w.data)
                return 4;
        }
        switch (w.kind)
        {
        case 1: w.options.flags ^= cvtt::Flags::BC7_FastIndexing; break;
        case 2: w.options.threshold = 0.25f; break;
        case 3: w.options.redWeight = 0.5f; break;
        case 4: w.options.greenWeight = 0.5f; break;
        case 5: w.options.blueWeight = 0.5f; break;
        case 6: w.options.alphaWeight = 0.5f; break;
        case 7: w.options.refineRoundsBC7 = 1; break;
        case 8: w.options.seedPoints = 2; break;
        case 9: w.plan.mode6Enabled = false; break;
        default: break;
        }
    }
    Barrier barrier(kNumThreads);
    std::vector<std::thread> threads;
    for (int t = 0; t < kNumThreads; t++)
        threads.push_back(std::thread(threadBody, &work[t], repetitions, &barrier));
    for (int t = 0; t < kNumThreads; t++)
        threads[t].join();
    for (int t = 0; t < kNumThreads; t++)
        if (work[t].data)
            K::ReleaseETC2Data(work[t].data, ledgerFree);
    for (int t = 0; t < kNumThreads; t++)
    {
        char name[16];
        snprintf(name, sizeof(name), "t%02d", t);
        emitNum("threads", "differing_repetitions", kKindNames[work[t].kind], name, work[t].differing);
    }
    for (int t = 0; t < kNumThreads; t++)
    {
        char name[16];
        snprintf(name, sizeof(name), "t%02d", t);
        emitHex("threads", "final", kKindNames[work[t].kind], name, work[t].last, 192);
    }
    emitNum("threads", "Release", "-", "mismatches", ledgerMismatches() + ledgerLive());
    return 0;
}

int main(int argc, char **argv)
{
    printf("source_sha %s\n", STR(CLIENT_SRC_SHA));
    if (argc < 2)
    {
        fprintf(stderr, "usage: %s host|s3tc|bc7|bc6h|etc|eac|decode|batch|threads [repetitions]\n", argv[0]);
        return 2;
    }
    if (contentSelfCheck() != 0)
        return 3;
    const std::string section = argv[1];
    int rc = 2;
    if (section == "host") rc = sectionHost();
    else if (section == "s3tc") rc = sectionS3TC();
    else if (section == "bc7") rc = sectionBC7();
    else if (section == "bc6h") rc = sectionBC6H();
    else if (section == "etc") rc = sectionETC();
    else if (section == "eac") rc = sectionEAC();
    else if (section == "decode") rc = sectionDecode();
    else if (section == "batch") rc = sectionBatch();
    else if (section == "threads") rc = sectionThreads(argc > 2 ? atoi(argv[2]) : 1);
    else fprintf(stderr, "unknown section %s\n", argv[1]);
    fflush(stdout);
    return rc;
}
