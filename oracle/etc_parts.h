/* TEST INFRASTRUCTURE ONLY -- the domains of the ETC part sweeps (tests/etc_parts.py), shared by the three sides that
 * walk them: the restatement (cvtt_oracle.c, orc_etc_parts), the reference's own functions (ref_etc_parts.cpp) and the
 * device (tests/device/lanetest_etc.hip).  Plain C that is also C++ and HIP.  Nothing here computes what is under test:
 * this file turns an input number into the arguments of a part and packs a part's result into one word.
 *
 * A sweep is (part, variant, three weights, a table of words); its inputs are numbered 0 ... 4096 * chunks - 1 and
 * input n belongs to chunk n >> 12.  A chunk's 4096 results fold into one checksum, the scheme of
 * tests/device/lanetest_checksum.h restated in C (etcp_term). */
#ifndef CVTT_ETC_PARTS_H
#define CVTT_ETC_PARTS_H
#include <stdint.h>

#ifdef __HIPCC__
#define ETCP_FN __host__ __device__ static inline
#else
#define ETCP_FN static inline
#endif

enum
{
    ETCP_RESOLVE_TH = 0, /* the three quantised channels after the resolver, bit 31: a channel outside 0 ... 15 */
    ETCP_RESOLVE_HALF,   /* variant bit 0: differential, bit 1: accurate; bit 31: a channel outside etcp_half_limit */
    ETCP_ERR_FAKE,       /* the float's bits */
    ETCP_ERR_WU,         /* variant 0: uniform, 1: weighted */
    ETCP_ERR2,           /* two colours at once on the device, the weighted scalar form elsewhere; variant: which of the two */
    ETCP_PLANAR,         /* planarDecode(coeff, ch) */
    ETCP_EMIT_T,         /* variant bit 0: the low word, bit 1: the sample with a channel at 16 */
    ETCP_EMIT_H,         /* variant bit 0: the low word, bit 1: the sample with a 5-bit field above 15 */
    ETCP_PARTS
};

#define ETCP_CHUNK 4096u
#define ETCP_TH_VALUES 128     /* targets per channel and granularity: table[16][128] */
#define ETCP_HALF_VALUES 256   /* candidates of the third channel: table[256]; an input takes one of 64 of them */
#define ETCP_PIXELS 64         /* table: int px[64][3], then the bits of float pw[64][3] */
#define ETCP_FLAG 0x80000000u

ETCP_FN uint32_t etcp_chunks(int part, int variant)
{
    switch (part)
    {
    case ETCP_RESOLVE_TH: return (16u << 21) / ETCP_CHUNK;
    case ETCP_RESOLVE_HALF: return (1u << 28) / ETCP_CHUNK;
    case ETCP_ERR_FAKE:
    case ETCP_ERR_WU:
    case ETCP_ERR2: return (1u << 30) / ETCP_CHUNK;
    case ETCP_PLANAR: return 1u;
    case ETCP_EMIT_T:
    case ETCP_EMIT_H: return ((variant & 2) ? (1u << 20) : (1u << 28)) / ETCP_CHUNK;
    }
    return 0;
}

ETCP_FN uint64_t etcp_term(uint32_t r, uint32_t j)
{
    return (uint64_t)(r ^ (j * 0x9E3779B1u)) * (0x9E3779B97F4A7C15ull + 2ull * j);
}

ETCP_FN uint32_t etcp_hash(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

ETCP_FN uint32_t etcp_float_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : u; /* no input of these domains gives a NaN; if one did, its payload is not compared */
}

ETCP_FN float etcp_bits_float(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

ETCP_FN uint32_t etcp_pack3(const int q[3], int limit)
{
    const int bad = q[0] < 0 || q[0] > limit || q[1] < 0 || q[1] > limit || q[2] < 0 || q[2] > limit;
    return ((uint32_t)q[0] & 255u) | (((uint32_t)q[1] & 255u) << 8) | (((uint32_t)q[2] & 255u) << 16) | (bad ? ETCP_FLAG : 0u);
}

/* the field of resolveHalfFake's result: 0 ... 31 differential, 0 ... 15 individual; variant bit 2 holds the differential form
 * to the individual field (only to see the flag raised) */
ETCP_FN int etcp_half_limit(int variant) { return ((variant & 1) && !(variant & 4)) ? 31 : 15; }

/* resolveTHFake: n = (granularity - 1) << 21 | i2 << 14 | i1 << 7 | i0, the target of channel ch = table[granularity - 1][i_ch],
 * the quantised value as the callers derive it */
ETCP_FN void etcp_th_args(const int32_t *table, uint32_t n, int *granularity, int targets[3], int quantized[3])
{
    const int g = (int)((n >> 21) & 15u) + 1;
    *granularity = g;
    for (int ch = 0; ch < 3; ch++)
    {
        const int t = table[(g - 1) * ETCP_TH_VALUES + (int)((n >> (7 * ch)) & 127u)];
        const int d = t / (34 * g);
        targets[ch] = t;
        quantized[ch] = d < 15 ? d : 15;
    }
}

/* resolveHalfFake: n = c0 << 17 | c1 << 6 | i; c0, c1 = every value 0 ... 2040 (above: 2040 again), c2 = one of the 256
 * candidates: four neighbouring pairs take all of them */
ETCP_FN void etcp_half_args(const int32_t *table, uint32_t n, int cumulative[3])
{
    const int c0 = (int)((n >> 17) & 2047u), c1 = (int)((n >> 6) & 2047u), i = (int)(n & 63u);
    cumulative[0] = c0 < 2040 ? c0 : 2040;
    cumulative[1] = c1 < 2040 ? c1 : 2040;
    cumulative[2] = table[i * 4 + ((c0 + c1) & 3)];
}

/* the metrics: n = colour << 6 | pixel, colour = r << 16 | g << 8 | b */
ETCP_FN void etcp_err_args(const int32_t *table, uint32_t n, int rec[3], int px[3], float pw[3])
{
    const uint32_t colour = (n >> 6) & 0xffffffu, p = n & 63u;
    rec[0] = (int)(colour >> 16);
    rec[1] = (int)((colour >> 8) & 255u);
    rec[2] = (int)(colour & 255u);
    for (int ch = 0; ch < 3; ch++)
    {
        px[ch] = table[p * 3 + ch];
        pw[ch] = etcp_bits_float((uint32_t)table[ETCP_PIXELS * 3 + p * 3 + ch]);
    }
}

/* the colour that shares the pair with colour n >> 6 (ETCP_ERR2) */
ETCP_FN void etcp_err2_partner(uint32_t n, int rec[3])
{
    const uint32_t colour = etcp_hash((n >> 6) ^ 0x2545f491u) & 0xffffffu;
    rec[0] = (int)(colour >> 16);
    rec[1] = (int)((colour >> 8) & 255u);
    rec[2] = (int)(colour & 255u);
}

typedef struct
{
    int line[3], iso[3];
    uint32_t selectors;
    int table, opaque;
} etcp_t_args;

typedef struct
{
    int bc[2];
    uint32_t sector, sign;
    int table, opaque;
} etcp_h_args;

/* the selector patterns of the emitters: 0 = every value in the block, 1 = one value only, 2 and 3 seeded */
ETCP_FN uint32_t etcp_t_selectors(uint32_t n, int pattern)
{
    const uint32_t h = etcp_hash(n ^ 0x51ed270bu);
    if (pattern == 0)
    {
        const int rot = 2 * (int)(h & 15u);
        return rot ? (0x1b1b1b1bu << rot) | (0x1b1b1b1bu >> (32 - rot)) : 0x1b1b1b1bu;
    }
    if (pattern == 1)
        return (h & 3u) * 0x55555555u;
    return etcp_hash(h + (uint32_t)pattern);
}

/* (sector, sign) of the H emitter: 0 = the four combinations in the block, 1 = one combination only, 2 and 3 seeded */
ETCP_FN void etcp_h_bits(uint32_t n, int pattern, uint32_t *sector, uint32_t *sign)
{
    const uint32_t h = etcp_hash(n ^ 0x3c6ef372u);
    if (pattern == 0)
    {
        *sector = (h & 1u) ? 0x5a3cu : 0xa5c3u;
        *sign = (h & 2u) ? 0x6996u : 0x9669u;
    }
    else if (pattern == 1)
    {
        *sector = (h & 1u) ? 0xffffu : 0u;
        *sign = (h & 2u) ? 0xffffu : 0u;
    }
    else
    {
        const uint32_t s = etcp_hash(h + (uint32_t)pattern);
        *sector = s & 0xffffu;
        *sign = s >> 16;
    }
}

ETCP_FN int etcp_pattern_of(uint32_t n) { return (int)((etcp_hash(n + 0x68e31da4u) >> 9) & 3u); }

/* emitT: n = opaque << 27 | table << 24 | isolated (r, g, b: 4 bits each) << 12 | line (r, g, b).  `wide`: n < 2^20 seeds
 * six channels 0 ... 16 of which at least one is 16 */
ETCP_FN void etcp_t_args_of(uint32_t n, int wide, int pattern, etcp_t_args *a)
{
    if (!wide)
    {
        for (int ch = 0; ch < 3; ch++)
        {
            a->line[ch] = (int)((n >> (4 * ch)) & 15u);
            a->iso[ch] = (int)((n >> (12 + 4 * ch)) & 15u);
        }
        a->table = (int)((n >> 24) & 7u);
        a->opaque = (int)((n >> 27) & 1u);
    }
    else
    {
        const uint32_t h1 = etcp_hash(n), h2 = etcp_hash(n + 0x9e3779b9u);
        int v[6];
        for (int i = 0; i < 6; i++)
            v[i] = (int)(((h1 >> (5 * i)) & 31u) % 17u);
        v[h2 % 6u] = 16;
        for (int ch = 0; ch < 3; ch++)
        {
            a->line[ch] = v[ch];
            a->iso[ch] = v[3 + ch];
        }
        a->table = (int)((h2 >> 8) & 7u);
        a->opaque = (int)((h2 >> 11) & 1u);
    }
    a->selectors = etcp_t_selectors(n, pattern);
}

/* emitH: n = opaque << 27 | table << 24 | colour 1 << 12 | colour 0 (r << 8 | g << 4 | b), handed over in the callers' packed
 * form r << 10 | g << 5 | b.  `wide`: n < 2^20 seeds two 15-bit colours of which at least one field is above 15; one
 * input in eight repeats the first colour */
ETCP_FN void etcp_h_args_of(uint32_t n, int wide, int pattern, etcp_h_args *a)
{
    if (!wide)
    {
        for (int s = 0; s < 2; s++)
        {
            const uint32_t c = (n >> (12 * s)) & 0xfffu;
            a->bc[s] = (int)(((c >> 8) << 10) | (((c >> 4) & 15u) << 5) | (c & 15u));
        }
        a->table = (int)((n >> 24) & 7u);
        a->opaque = (int)((n >> 27) & 1u);
    }
    else
    {
        const uint32_t h1 = etcp_hash(n), h2 = etcp_hash(n + 0x9e3779b9u);
        const uint32_t f = h2 % 6u;
        a->bc[0] = (int)(h1 & 0x7fffu);
        a->bc[1] = (int)((h1 >> 15) & 0x7fffu);
        a->bc[f / 3u] |= 16 << (5 * (int)(f % 3u));
        if (((h2 >> 12) & 7u) == 0)
            a->bc[1] = a->bc[0];
        a->table = (int)((h2 >> 8) & 7u);
        a->opaque = (int)((h2 >> 11) & 1u);
    }
    etcp_h_bits(n, pattern, &a->sector, &a->sign);
}

#endif
