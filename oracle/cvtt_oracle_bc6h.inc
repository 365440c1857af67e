/* TEST INFRASTRUCTURE ONLY -- BC6H (BC6HComputer::Pack) restatement, included by cvtt_oracle.c.
 * Follows ConvectionKernels_BC67.cpp:2425-3051, ConvectionKernels_IndexSelectorHDR.h,
 * ConvectionKernels_UnfinishedEndpoints.h:39-75, ConvectionKernels_EndpointRefiner.h:154-175,
 * ParallelMath.h:996-1066.  The 8 lanes of a group run in lock-step: the duplicate-round skip
 * (BC67.cpp:2853-2877, AllSet) and the mode commit loop (2936-2984, AnySet) couple them.
 * Canonical oracle semantics (SURVEY App. C): automatics start zeroed, statements execute in
 * program order with respect to the MXCSR rounding scopes. */
#include "cvtt_oracle_bc6h_layout.h"
#include <fenv.h>
#include <stdio.h>

/* RCPPS-free helpers for the round-up scope of BC67.cpp:2509, 2556 */
static float hdr_div_ru(float a, float b)
{
    volatile float va = a, vb = b, r;
    fesetround(FE_UPWARD);
    r = va / vb;
    fesetround(FE_TONEAREST);
    return r;
}

/* QuantizeSingleEndpointElementUnsigned, BC67.cpp:2441-2445 */
static int bc6h_quantize_unsigned(int elem, int precision)
{
    float v = hdr_div_ru((float)elem * 64.0f, 31.0f);
    v = f_min(v, 65535.0f);
    /* RoundAndConvertToU16 under round-up: cvtps2dq(v - 32768) -> pack -> ^0x8000 == ceil(v) */
    int i = (int)ceilf(v - 32768.0f);
    if (i > 32767) i = 32767;
    if (i < -32768) i = -32768;
    unsigned expanded = ((unsigned)(i & 0xffff)) ^ 0x8000u;
    return (int)((expanded & 0xffffu) >> (16 - precision));
}

/* QuantizeSingleEndpointElementSigned, BC67.cpp:2425-2439 */
static int bc6h_quantize_signed(int elem2CL, int precision)
{
    int isNegative = elem2CL < 0;
    int absElem = isNegative ? -elem2CL : elem2CL;
    float v = hdr_div_ru((float)absElem * 32.0f, 31.0f);
    int i = (int)ceilf(v); /* RoundAndConvertToU15 under round-up, signed saturating pack */
    if (i > 32767) i = 32767;
    absElem = (int)(((unsigned)i & 0xffffu) >> (16 - precision));
    return isNegative ? -absElem : absElem;
}

/* UnquantizeSingleEndpointElementUnsigned, BC67.cpp:2482-2501 */
static void bc6h_unquantize_unsigned(int comp, int precision, int *outUnq, int *outFinished)
{
    unsigned unq = (unsigned)comp & 0xffffu;
    if (precision < 15)
    {
        int isZero = comp == 0;
        int isMax = ((1 << precision) - 2) < comp;
        unq = ((unsigned)(comp << (16 - precision)) + (0x8000u >> precision)) & 0xffffu;
        if (isZero) unq = 0;
        if (isMax) unq = 0xffff;
    }
    *outUnq = (int)unq;
    *outFinished = (int)(((unq * 31u) >> 6) & 0xffffu);
}

/* UnquantizeSingleEndpointElementSigned, BC67.cpp:2447-2480 */
static void bc6h_unquantize_signed(int comp, int precision, int *outUnq, int *outFinished2CL)
{
    int negative = comp < 0;
    int absComp = negative ? -comp : comp;
    int unq, absUnq;
    if (precision >= 16)
    {
        unq = comp;
        absUnq = absComp;
    }
    else
    {
        int isZero = comp == 0;
        int isMax = ((1 << (precision - 1)) - 2) < comp;
        absUnq = (int)(int16_t)(uint16_t)((absComp << (16 - precision)) + (0x4000 >> (precision - 1)));
        if (isZero) absUnq = 0;
        if (isMax) absUnq = 0x7fff;
        unq = negative ? -absUnq : absUnq;
    }
    *outUnq = (int)(int16_t)unq;
    int funq = (int)(((unsigned)(absUnq & 0xffff) * 31u) >> 5);
    if (funq > 32767) funq = 32767; /* ToUInt15: saturating pack */
    *outFinished2CL = (int)(int16_t)(negative ? -funq : funq);
}

/* TwosCLHalfToFloat, ParallelMath.h:1012-1041 (16-bit lane ops, then a float subtract) */
static float twos_cl_half_to_float(int v16)
{
    uint16_t v = (uint16_t)v16;
    uint16_t signBits = v & 0x8000u;
    uint16_t mantissa = v & 0x03ffu;
    uint16_t exponent = v & 0x7c00u;
    int isDenormal = exponent == 0;
    exponent = (uint16_t)((exponent >> 3) + 14336);
    uint16_t denormalCorrectionHigh = isDenormal ? (uint16_t)(signBits | 14336) : 0;
    uint16_t highBits = (uint16_t)(signBits | exponent | (mantissa >> 3));
    uint16_t lowBits = (uint16_t)(mantissa << 13);
    uint32_t fbits = ((uint32_t)highBits << 16) | lowBits;
    uint32_t cbits = (uint32_t)denormalCorrectionHigh << 16;
    float f, c;
    memcpy(&f, &fbits, 4);
    memcpy(&c, &cbits, 4);
    return f - c;
}

typedef struct
{
    int range;
    int ep[2][3];    /* interpolation endpoints (unquantized), 16-bit abstract */
    float origin[3]; /* colour-space endpoints */
    float axis[3];
    float maxValue;
    float interp[16][3]; /* m_reconstructedInterpolators (slow indexing) */
    int isInverted;
} hdr_selector_t;

/* UnscaleHDRValueSigned / Unsigned, BC67.cpp:766-787 */
static int unscale_hdr_signed(int v)
{
    int negative = v < 0;
    int absComp = negative ? -v : v;
    int scaled = (int)(((unsigned)(absComp & 0xffff) * 31u) >> 5);
    if (scaled > 32767) scaled = 32767;
    return (int)(int16_t)(uint16_t)((unsigned)scaled | (negative ? 0x8000u : 0u));
}
static int unscale_hdr_unsigned(int v) { return (int)((((unsigned)v & 0xffffu) * 31u) >> 6); }

/* ReconstructHDR{Signed,Unsigned}Uninverted, IndexSelectorHDR.h:34-66 */
static void hdr_reconstruct_uninverted(const hdr_selector_t *s, int index, int isSigned, int pixel[3])
{
    uint16_t weight = (uint16_t)((uint16_t)((uint16_t)(weight_reciprocal(s->range) * (unsigned)index) + 256) >> 9);
    for (int ch = 0; ch < 3; ch++)
    {
        if (isSigned)
        {
            int32_t e0 = (int16_t)s->ep[0][ch], e1 = (int16_t)s->ep[1][ch];
            int32_t p = (int32_t)(64 - weight) * e0 + (int32_t)weight * e1;
            p = (p + 32) >> 6;
            if (p > 32767) p = 32767;
            if (p < -32768) p = -32768;
            pixel[ch] = unscale_hdr_signed(p);
        }
        else
        {
            uint32_t e0 = (uint16_t)s->ep[0][ch], e1 = (uint16_t)s->ep[1][ch];
            uint32_t p = (uint32_t)(64 - weight) * e0 + (uint32_t)weight * e1;
            p = (p + 32) >> 6;
            pixel[ch] = (int)(int16_t)unscale_hdr_unsigned((int)(p & 0xffffu));
        }
    }
}

static inline int hdr_invert_single(const hdr_selector_t *s, int index)
{
    return s->isInverted ? (s->range - 1) - index : index;
}

/* IndexSelector::Init + InitHDR, IndexSelector.h:27-77, IndexSelectorHDR.h:84-108 */
static void hdr_selector_init(hdr_selector_t *s, const float *w, const int interp[2][3], const int colorSpace[2][3],
                              int colorSpaceUnsigned16, int range, int isSigned, int fastIndexing)
{
    float epDW[3];
    s->range = range;
    s->maxValue = (float)(range - 1);
    for (int ch = 0; ch < 3; ch++)
    {
        s->ep[0][ch] = interp[0][ch];
        s->ep[1][ch] = interp[1][ch];
        float c0 = colorSpaceUnsigned16 ? (float)(colorSpace[0][ch] & 0xffff) : (float)(int16_t)colorSpace[0][ch];
        float c1 = colorSpaceUnsigned16 ? (float)(colorSpace[1][ch] & 0xffff) : (float)(int16_t)colorSpace[1][ch];
        s->origin[ch] = c0;
        epDW[ch] = (c1 - c0) * w[ch];
    }
    float lenSq = epDW[0] * epDW[0];
    lenSq = lenSq + epDW[1] * epDW[1];
    lenSq = lenSq + epDW[2] * epDW[2];
    lenSq = f_safe_denom(lenSq);
    float mvdls = s->maxValue / lenSq;
    for (int ch = 0; ch < 3; ch++)
        s->axis[ch] = epDW[ch] * w[ch] * mvdls;
    s->isInverted = 0;
    if (!fastIndexing)
    {
        for (int i = 0; i < range; i++)
        {
            int recon[3];
            hdr_reconstruct_uninverted(s, i, isSigned, recon);
            for (int ch = 0; ch < 3; ch++)
                s->interp[i][ch] = twos_cl_half_to_float(recon[ch]) * w[ch];
        }
    }
}

/* SelectIndexHDRSlow / Fast, IndexSelectorHDR.h:125-144 */
static int hdr_select_slow(const hdr_selector_t *s, const float *pixel)
{
    int index = 0;
    float bestError;
    {
        float d = pixel[0] - s->interp[0][0];
        bestError = d * d;
        for (int ch = 1; ch < 3; ch++)
        {
            d = pixel[ch] - s->interp[0][ch];
            bestError = bestError + d * d;
        }
    }
    for (int i = 1; i < s->range; i++)
    {
        float d = pixel[0] - s->interp[i][0];
        float error = d * d;
        for (int ch = 1; ch < 3; ch++)
        {
            d = pixel[ch] - s->interp[i][ch];
            error = error + d * d;
        }
        if (error < bestError)
            index = i;
        bestError = f_min(bestError, error);
    }
    return hdr_invert_single(s, index);
}

static int hdr_select_fast(const hdr_selector_t *s, const float *pixel)
{
    float dist = (pixel[0] - s->origin[0]) * s->axis[0];
    for (int ch = 1; ch < 3; ch++)
        dist = dist + (pixel[ch] - s->origin[ch]) * s->axis[ch];
    return hdr_invert_single(s, cvt_rne_s16(f_clamp(dist, 0.0f, s->maxValue)));
}

/* BCCommon::ComputeErrorHDRFast / Slow, BCCommon.h:45-79 */
static float hdr_error(uint32_t flags, int fast, const int rec[3], const int16_t orig[3], const float *wSq)
{
    float error = 0.0f;
    for (int ch = 0; ch < 3; ch++)
    {
        float sq;
        if (fast)
        {
            /* SqDiffSInt16, ParallelMath.h:996-1010: unsigned 16-bit difference, 32-bit square
             * converted as a SIGNED 32-bit integer */
            int a = (int16_t)rec[ch], b = orig[ch];
            uint32_t diffU = (uint16_t)((a > b ? a : b) - (a > b ? b : a));
            uint32_t prod = diffU * diffU;
            sq = (float)(int32_t)prod;
        }
        else
        {
            float d = twos_cl_half_to_float(rec[ch]) - twos_cl_half_to_float(orig[ch]);
            sq = d * d;
        }
        if (flags & ORC_FLAG_UNIFORM)
            error = error + sq;
        else
            error = error + sq * wSq[ch];
    }
    return error;
}

#ifdef ORC_BC6H_STATS
/* developer instrumentation (tools/bc6h_search_stats.py): what the search does per precision */
enum { ST_ROUNDS, ST_GROUPDUP, ST_LANEROUNDS, ST_LANEDUP, ST_LANEDUP_EXACT, ST_OWNFIT0, ST_LANEPART, ST_LANEPART_CANBEAT,
       ST_LANEPART_COMMIT, ST_COMMITS, ST_PAIRS_BETTER, ST_PAIRS_BETTER_LEGAL, ST_GROUPPART, ST_GROUPPART_CANBEAT, ST_GROUPPART_COMMIT, ST_N };
unsigned long long orc_bc6h_stats[17][ST_N];
#define STAT(prec, k, n) (orc_bc6h_stats[prec][k] += (n))
#else
#define STAT(prec, k, n) ((void)0)
#endif

typedef struct
{
    int16_t pixels[16][3];
    float floatPixels2CL[16][3];
    float floatPixelsLinearWeighted[16][3];
    float preWeighted[16][3];
    unfinished_t partitionedUFEP[32][2];
    unfinished_t singleUFEP;
    int bestEndPoints[2][2][3];
    int bestIndexes[16];
    float bestError;
    int bestMode, bestPartition;
    /* per (precision, partition) */
    int metaEPQ[12][2][2][3];
    int metaIndexes[12][16];
    float metaError[12][2];
    /* per tweak */
    refiner_t refiners[2];
    hdr_selector_t sel;
    int anySame;
#ifdef ORC_BC6H_STATS
    int preSwap[12][2][2][3], inv[12][2], dupExact, commitsHere;
#endif
} bc6h_lane_t;

/* EndpointRefiner::GetRefinedEndpointsHDR, EndpointRefiner.h:154-175 */
static void refiner_get_hdr(const refiner_t *r, int ep[2][3], int isSigned)
{
    float fe[2][4];
    refiner_solve(r, fe);
    for (int epi = 0; epi < 2; epi++)
        for (int ch = 0; ch < 3; ch++)
        {
            float f = fe[epi][ch];
            if (isSigned)
                ep[epi][ch] = cvt_rne_s16(f_clamp(f, -31743.0f, 31743.0f));
            else
                ep[epi][ch] = cvt_rne_s16(f_clamp(f, 0.0f, 31743.0f));
        }
}

/* QuantizeEndpoints{Signed,Unsigned}, BC67.cpp:2503-2595 (one lane) */
static void bc6h_quantize_endpoints(bc6h_lane_t *ln, const int endPoints[2][3], int quantized[2][3], int *indexes,
                                    int fixupIndex, int precision, int indexRange, const float *w, int fastIndexing,
                                    int isSigned)
{
    int unq[2][3], finished[2][3];
    for (int epi = 0; epi < 2; epi++)
        for (int ch = 0; ch < 3; ch++)
        {
            int qee;
            if (isSigned)
            {
                qee = bc6h_quantize_signed(endPoints[epi][ch], precision);
                bc6h_unquantize_signed(qee, precision, &unq[epi][ch], &finished[epi][ch]);
            }
            else
            {
                qee = bc6h_quantize_unsigned(endPoints[epi][ch] & 0xffff, precision);
                bc6h_unquantize_unsigned(qee, precision, &unq[epi][ch], &finished[epi][ch]);
            }
            quantized[epi][ch] = (int)(int16_t)qee;
        }
    hdr_selector_init(&ln->sel, w, unq, finished, !isSigned, indexRange, isSigned, fastIndexing);

    int index = fastIndexing ? hdr_select_fast(&ln->sel, ln->floatPixels2CL[fixupIndex])
                             : hdr_select_slow(&ln->sel, ln->floatPixelsLinearWeighted[fixupIndex]);
    int invert = (indexRange / 2 - 1) < index;
    if (invert)
    {
        index = (indexRange - 1) - index;
        for (int ch = 0; ch < 3; ch++)
        {
            int t = quantized[0][ch];
            quantized[0][ch] = quantized[1][ch];
            quantized[1][ch] = t;
        }
    }
    ln->sel.isInverted = invert;
    indexes[fixupIndex] = index;
}

/* Evaluate{Partitioned,Single}Legality, BC67.cpp:2597-2663 (one lane) */
static int bc6h_legality(const int ep0[2][3], const int ep1[2][3], int partitioned, int aPrec, const uint8_t *bPrec,
                         int transformed, int outEncoded[2][2][3])
{
    int legal = 1;
    const int mask = (1 << aPrec) - 1;
    const int numSubsets = partitioned ? 2 : 1;
    for (int ch = 0; ch < 3; ch++)
    {
        outEncoded[0][0][ch] = ep0[0][ch];
        outEncoded[0][1][ch] = ep0[1][ch];
        if (partitioned)
        {
            outEncoded[1][0][ch] = ep1[0][ch];
            outEncoded[1][1][ch] = ep1[1][ch];
        }
        if (transformed)
        {
            for (int subset = 0; subset < numSubsets; subset++)
                for (int epi = 0; epi < 2; epi++)
                {
                    if (epi == 0 && subset == 0)
                        continue;
                    int bReduced = outEncoded[subset][epi][ch] & mask & 0xffff;
                    int16_t d16 = (int16_t)(uint16_t)(outEncoded[subset][epi][ch] - outEncoded[0][0][ch]);
                    int lost = 16 - bPrec[ch];
                    int16_t delta = lost ? (int16_t)((int16_t)(uint16_t)((uint16_t)d16 << lost) >> lost) : d16;
                    outEncoded[subset][epi][ch] = delta;
                    int reconstructed = (uint16_t)(delta + outEncoded[0][0][ch]) & mask & 0xffff;
                    legal = legal && (reconstructed == bReduced);
                }
        }
    }
    return legal;
}

static void bc6h_emit(const bc6h_lane_t *ln, uint8_t *out)
{
    const int mode = ln->bestMode;
    const uint8_t *mi = orc_bc6h_mode_info[mode];
    const int partitioned = mi[1];
    const int headerBits = partitioned ? 82 : 65;
    unsigned fields[14];
    fields[0] = mi[0];
    fields[1] = (unsigned)ln->bestPartition;
    for (int ch = 0; ch < 3; ch++)
    {
        fields[2 + ch * 4 + 0] = (unsigned)ln->bestEndPoints[0][0][ch] & 0xffffu;
        fields[2 + ch * 4 + 1] = (unsigned)ln->bestEndPoints[0][1][ch] & 0xffffu;
        fields[2 + ch * 4 + 2] = (unsigned)ln->bestEndPoints[1][0][ch] & 0xffffu;
        fields[2 + ch * 4 + 3] = (unsigned)ln->bestEndPoints[1][1][ch] & 0xffffu;
    }
    packer_t pv;
    pk_init(&pv); /* canonical oracle: the packing words start at zero (hazard H1) */
    for (int bit = 0; bit < headerBits; bit++)
    {
        int code = orc_bc6h_header_layout[mode][bit];
        pk_pack(&pv, (fields[code >> 4] >> (code & 15)) & 1u, 1);
    }
    int fixupIndex1 = 0, indexBits = 4;
    if (partitioned)
    {
        fixupIndex1 = orc_anchor2[ln->bestPartition];
        indexBits = 3;
    }
    for (int px = 0; px < 16; px++)
    {
        if (px == 0 || px == fixupIndex1)
            pk_pack(&pv, (unsigned)ln->bestIndexes[px], indexBits - 1);
        else
            pk_pack(&pv, (unsigned)ln->bestIndexes[px], indexBits);
    }
    pk_flush(&pv, out);
}

static const uint8_t bc6h_modes_exist[2][17] = {
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1},
    {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
};

/* BC6HComputer::Pack for one group, BC67.cpp:2665-3051 */
static void bc6h_encode_group(const uint8_t *blocksBytes, uint8_t *out, const orc_options *options, int isSigned,
                              const float *rcp, uint32_t siteMask, int siteLane)
{
    static __thread bc6h_lane_t lanes[8];
    const uint32_t flags = options->flags;
    int numTweakRounds = options->seedPoints;
    int numRefineRounds = options->refineRoundsBC6H;
    if (numTweakRounds < 1) numTweakRounds = 1; else if (numTweakRounds > 4) numTweakRounds = 4;
    if (numRefineRounds < 1) numRefineRounds = 1; else if (numRefineRounds > 3) numRefineRounds = 3;
    const int fastIndexing = (flags & ORC_FLAG_BC6H_FAST_INDEXING) != 0;
    float w[4], wSq[3];
    fill_weights(options, w);
    for (int ch = 0; ch < 3; ch++)
        wSq[ch] = w[ch] * w[ch];
    const int16_t *in = (const int16_t *)blocksBytes;

    for (int l = 0; l < 8; l++)
    {
        bc6h_lane_t *ln = &lanes[l];
        for (int px = 0; px < 16; px++)
            for (int ch = 0; ch < 3; ch++)
            {
                int v = in[(l * 16 + px) * 4 + ch];
                if (isSigned)
                {
                    int negative = v < 0;
                    int magnitude = v & 32767;
                    if (negative) v = -magnitude;
                    if (v < -31743) v = -31743;
                }
                else if (v < 0)
                    v = 0;
                if (v > 31743) v = 31743;
                ln->pixels[px][ch] = (int16_t)v;
                ln->floatPixels2CL[px][ch] = (float)v;
                ln->floatPixelsLinearWeighted[px][ch] = twos_cl_half_to_float(v) * w[ch];
                ln->preWeighted[px][ch] = (float)v * w[ch];
            }
        memset(ln->bestEndPoints, 0, sizeof(ln->bestEndPoints));
        memset(ln->bestIndexes, 0, sizeof(ln->bestIndexes));
        ln->bestError = FLT_MAX;
        ln->bestMode = 0;
        ln->bestPartition = 0;
        for (int p = 0; p < 32; p++)
        {
            uint8_t frag[2][16];
            int len[2] = {0, 0};
            for (int px = 0; px < 16; px++)
            {
                int s = (orc_partition2[p] >> px) & 1;
                frag[s][len[s]++] = (uint8_t)px;
            }
            for (int s = 0; s < 2; s++)
                pca_endpoints(&ln->preWeighted[0][0], 3, 3, frag[s], len[s], w, &ln->partitionedUFEP[p][s]);
        }
        pca_endpoints(&ln->preWeighted[0][0], 3, 3, NULL, 16, w, &ln->singleUFEP);
    }

    for (int partitionedInt = 0; partitionedInt < 2; partitionedInt++)
    {
        const int partitioned = partitionedInt == 1;
        for (int aPrec = 16; aPrec >= 0; aPrec--)
        {
            if (!bc6h_modes_exist[partitionedInt][aPrec])
                continue;
            const int numPartitions = partitioned ? 32 : 1;
            const int numSubsets = partitioned ? 2 : 1;
            const int indexBits = partitioned ? 3 : 4;
            const int indexRange = 1 << indexBits;

            for (int p = 0; p < numPartitions; p++)
            {
                const int partitionMask = partitioned ? orc_partition2[p] : 0;
                int roundValid[12][2];
                for (int r = 0; r < 12; r++)
                    roundValid[r][0] = roundValid[r][1] = 1;
                for (int l = 0; l < 8; l++)
                {
                    memset(lanes[l].metaEPQ, 0, sizeof(lanes[l].metaEPQ));
                    memset(lanes[l].metaIndexes, 0, sizeof(lanes[l].metaIndexes));
                    memset(lanes[l].metaError, 0, sizeof(lanes[l].metaError));
                }

                for (int subset = 0; subset < numSubsets; subset++)
                {
                    for (int tweak = 0; tweak < 4; tweak++)
                    {
                        for (int l = 0; l < 8; l++)
                        {
                            /* EndpointRefiner<3> refiners[2]: not constructed -> zero in the canonical build */
                            memset(lanes[l].refiners, 0, sizeof(lanes[l].refiners));
                            lanes[l].refiners[0].n = lanes[l].refiners[1].n = 3;
                            lanes[l].refiners[0].rcpLUT = lanes[l].refiners[1].rcpLUT = rcp;
                        }
                        int abortRemainingRefines = 0;
                        for (int refinePass = 0; refinePass < 3; refinePass++)
                        {
                            const int metaRound = tweak * 3 + refinePass;
                            if (tweak >= numTweakRounds || refinePass >= numRefineRounds)
                                abortRemainingRefines = 1;
                            if (abortRemainingRefines)
                            {
                                roundValid[metaRound][subset] = 0;
                                continue;
                            }
                            const int fixupIndex = (subset == 0) ? 0 : orc_anchor2[p];

                            int allSame = 1;
                            for (int l = 0; l < 8; l++)
                            {
                                bc6h_lane_t *ln = &lanes[l];
                                int endPointsColorSpace[2][3];
                                if (refinePass == 0)
                                {
                                    const unfinished_t *u = partitioned ? &ln->partitionedUFEP[p][subset] : &ln->singleUFEP;
                                    float tf[2];
                                    tweak_factors(tweak, indexRange, tf);
                                    for (int ch = 0; ch < 3; ch++)
                                        for (int epi = 0; epi < 2; epi++)
                                        {
                                            float lo = isSigned ? -31743.0f : 0.0f;
                                            float f = f_clamp(u->base[ch] + u->offset[ch] * tf[epi], lo, 31743.0f);
                                            endPointsColorSpace[epi][ch] = cvt_rne_s16(f);
                                        }
                                }
                                else
                                    refiner_get_hdr(&ln->refiners[subset], endPointsColorSpace, isSigned);

                                refiner_init(&ln->refiners[subset], 3, indexRange, w, rcp);
                                bc6h_quantize_endpoints(ln, endPointsColorSpace, ln->metaEPQ[metaRound][subset],
                                                        ln->metaIndexes[metaRound], fixupIndex, aPrec, indexRange, w,
                                                        fastIndexing, isSigned);
                                int anySame = 0;
#ifdef ORC_BC6H_STATS
                                ln->inv[metaRound][subset] = ln->sel.isInverted;
                                ln->dupExact = 0;
#endif
                                for (int prev = 0; prev < metaRound; prev++)
                                {
                                    int same = 1;
                                    for (int epi = 0; epi < 2; epi++)
                                        for (int ch = 0; ch < 3; ch++)
                                            same = same && ((int16_t)ln->metaEPQ[prev][subset][epi][ch] == (int16_t)ln->metaEPQ[metaRound][subset][epi][ch]);
                                    anySame = anySame || same;
#ifdef ORC_BC6H_STATS
                                    if (same && ln->inv[prev][subset] == ln->inv[metaRound][subset] && roundValid[prev][subset])
                                        ln->dupExact = 1;
#endif
                                }
                                ln->anySame = anySame;
                                allSame = allSame && anySame;
                            }
                            /* site switch: AllSet(anySame) answered by the viewing lane's own anySame: its round is
                             * dropped and its next refiner stays empty whenever IT repeats, whatever its mates do */
                            if (siteMask & ORC_SITE_BC6H_DUP_SKIP)
                                allSame = lanes[siteLane].anySame;
                            if (metaRound > 0 && allSame)
                            {
                                roundValid[metaRound][subset] = 0;
                                if (partitioned) STAT(aPrec, ST_GROUPDUP, 1);
                                continue;
                            }
#ifdef ORC_BC6H_STATS
                            if (partitioned)
                            {
                                STAT(aPrec, ST_ROUNDS, 1);
                                for (int l = 0; l < 8; l++)
                                {
                                    STAT(aPrec, ST_LANEROUNDS, 1);
                                    STAT(aPrec, ST_LANEDUP, metaRound > 0 && lanes[l].anySame);
                                    STAT(aPrec, ST_LANEDUP_EXACT, metaRound > 0 && lanes[l].dupExact);
                                    if (subset == 0)
                                    {
                                        int fit = 0;
                                        for (int mode = 0; mode < 14; mode++)
                                        {
                                            const uint8_t *mi = orc_bc6h_mode_info[mode];
                                            int enc[2][2][3];
                                            if (mi[1] != partitioned || mi[3] != aPrec) continue;
                                            /* own delta only: test with subset 1 = copies of ep0 (always fits) */
                                            fit = fit || bc6h_legality(lanes[l].metaEPQ[metaRound][0], (const int (*)[3])lanes[l].metaEPQ[metaRound][0], 0, mi[3], mi + 4, mi[2], enc);
                                        }
                                        STAT(aPrec, ST_OWNFIT0, fit);
                                    }
                                }
                            }
#endif

                            for (int l = 0; l < 8; l++)
                            {
                                bc6h_lane_t *ln = &lanes[l];
                                float subsetError = 0.0f;
                                for (int px = 0; px < 16; px++)
                                {
                                    if (subset != ((partitionMask >> px) & 1))
                                        continue;
                                    int index;
                                    if (px == fixupIndex)
                                        index = ln->metaIndexes[metaRound][px];
                                    else
                                    {
                                        index = fastIndexing ? hdr_select_fast(&ln->sel, ln->floatPixels2CL[px])
                                                             : hdr_select_slow(&ln->sel, ln->floatPixelsLinearWeighted[px]);
                                        ln->metaIndexes[metaRound][px] = index;
                                    }
                                    int reconstructed[3];
                                    hdr_reconstruct_uninverted(&ln->sel, hdr_invert_single(&ln->sel, index), isSigned, reconstructed);
                                    subsetError = subsetError + hdr_error(flags, fastIndexing, reconstructed, ln->pixels[px], wSq);
                                    if (refinePass != numRefineRounds - 1)
                                        refiner_contribute_unweighted(&ln->refiners[subset], ln->preWeighted[px], index, 3);
                                }
                                ln->metaError[metaRound][subset] = subsetError;
                            }
                        }
                    }
                }

#ifdef ORC_BC6H_STATS
                int gCan = 0;
                if (partitioned)
                    for (int l = 0; l < 8; l++)
                    {
                        float m0 = FLT_MAX, m1 = FLT_MAX;
                        for (int r = 0; r < 12; r++)
                        {
                            if (roundValid[r][0] && lanes[l].metaError[r][0] < m0) m0 = lanes[l].metaError[r][0];
                            if (roundValid[r][1] && lanes[l].metaError[r][1] < m1) m1 = lanes[l].metaError[r][1];
                        }
                        STAT(aPrec, ST_LANEPART, 1);
                        STAT(aPrec, ST_LANEPART_CANBEAT, m0 + m1 < lanes[l].bestError);
                        gCan = gCan || (m0 + m1 < lanes[l].bestError);
                        lanes[l].commitsHere = 0;
                    }
                if (partitioned) { STAT(aPrec, ST_GROUPPART, 1); STAT(aPrec, ST_GROUPPART_CANBEAT, gCan); }
#endif
#ifdef ORC_BC6H_TRACE
                /* developer trace (tools/bc6h_trace.py): the round history of lane ORC_BC6H_TRACE of the FIRST group at 6 bits */
                if (partitioned && aPrec == 6 && getenv("ORC_BC6H_TRACE_ON"))
                {
                    const bc6h_lane_t *tl = &lanes[ORC_BC6H_TRACE];
                    unsigned v0 = 0, v1 = 0;
                    for (int r = 0; r < 12; r++) { v0 |= (unsigned)roundValid[r][0] << r; v1 |= (unsigned)roundValid[r][1] << r; }
                    printf("TRACE p %d rv %x %x\n", p, v0, v1);
                    for (int s2 = 0; s2 < 2; s2++)
                        for (int r = 0; r < 12; r++)
                        {
                            union { float f; unsigned u; } cv;
                            cv.f = tl->metaError[r][s2];
                            printf("TRACE p %d s %d m %d ep %d %d %d %d %d %d err %08x\n", p, s2, r, tl->metaEPQ[r][s2][0][0], tl->metaEPQ[r][s2][0][1], tl->metaEPQ[r][s2][0][2],
                                   tl->metaEPQ[r][s2][1][0], tl->metaEPQ[r][s2][1][1], tl->metaEPQ[r][s2][1][2], cv.u);
                        }
                }
#endif
                /* delta-coding legality + commit, BC67.cpp:2914-2986 */
                const int numMeta1 = partitioned ? 12 : 1;
                for (int meta0 = 0; meta0 < 12; meta0++)
                {
                    if (!roundValid[meta0][0])
                        continue;
                    for (int meta1 = 0; meta1 < numMeta1; meta1++)
                    {
                        if (partitioned && !roundValid[meta1][1])
                            continue;
                        float combined[8];
                        int errorBetter[8], needsCommit[8], any = 0;
                        for (int l = 0; l < 8; l++)
                        {
                            combined[l] = lanes[l].metaError[meta0][0];
                            if (partitioned)
                                combined[l] = combined[l] + lanes[l].metaError[meta1][1];
                            errorBetter[l] = combined[l] < lanes[l].bestError;
                            needsCommit[l] = errorBetter[l];
                            any = any || errorBetter[l];
                        }
                        /* site switch: AnySet(errorBetter) / AnySet(needsCommit) answered by the viewing lane's own flags */
                        if (siteMask & ORC_SITE_BC6H_COMMIT_LOOP)
                            any = errorBetter[siteLane];
                        if (!any)
                            continue;
#ifdef ORC_BC6H_STATS
                        if (partitioned)
                            for (int l = 0; l < 8; l++)
                                STAT(aPrec, ST_PAIRS_BETTER, errorBetter[l]);
#endif
                        for (int mode = 0; mode < 14; mode++)
                        {
                            const uint8_t *mi = orc_bc6h_mode_info[mode];
                            if (mi[1] != partitioned || mi[3] != aPrec)
                                continue;
                            int anyCommit = 0, stillNeeds = 0;
                            for (int l = 0; l < 8; l++)
                            {
                                bc6h_lane_t *ln = &lanes[l];
                                int encoded[2][2][3];
                                memset(encoded, 0, sizeof(encoded));
                                int legal = bc6h_legality(ln->metaEPQ[meta0][0], ln->metaEPQ[meta1][1], partitioned, mi[3], mi + 4, mi[2], encoded);
                                int commit = errorBetter[l] && legal;
#ifdef ORC_BC6H_STATS
                                if (partitioned && commit) { STAT(aPrec, ST_COMMITS, 1); ln->commitsHere++; }
#endif
                                if (commit)
                                {
                                    if (!(siteMask & ORC_SITE_BC6H_COMMIT_LOOP) || l == siteLane)
                                        anyCommit = 1;
                                    ln->bestError = combined[l];
                                    ln->bestMode = mode;
                                    ln->bestPartition = p;
                                    for (int s = 0; s < numSubsets; s++)
                                        for (int epi = 0; epi < 2; epi++)
                                            for (int ch = 0; ch < 3; ch++)
                                                ln->bestEndPoints[s][epi][ch] = encoded[s][epi][ch];
                                    for (int px = 0; px < 16; px++)
                                    {
                                        int s = (partitionMask >> px) & 1;
                                        ln->bestIndexes[px] = s == 0 ? ln->metaIndexes[meta0][px] : ln->metaIndexes[meta1][px];
                                    }
                                    needsCommit[l] = 0;
                                }
                            }
                            for (int l = 0; l < 8; l++)
                                stillNeeds = stillNeeds || needsCommit[l];
                            if (siteMask & ORC_SITE_BC6H_COMMIT_LOOP)
                                stillNeeds = needsCommit[siteLane];
                            /* `continue` on no commit skips the needsCommit test (BC67.cpp:2954-2955) */
                            if (anyCommit && !stillNeeds)
                                break;
                        }
                    }
                }
#ifdef ORC_BC6H_STATS
                if (partitioned)
                {
                    int g = 0;
                    for (int l = 0; l < 8; l++) { STAT(aPrec, ST_LANEPART_COMMIT, lanes[l].commitsHere > 0); g = g || lanes[l].commitsHere > 0; }
                    STAT(aPrec, ST_GROUPPART_COMMIT, g);
                }
#endif
            }
        }
    }
    for (int l = 0; l < 8; l++)
        bc6h_emit(&lanes[l], out + l * 16);
}

static void bc6hu_group_thunk(const uint8_t *in, uint8_t *out, const void *a, const void *b, const float *rcp, size_t group)
{
    (void)group;
    ORC_RUN_SITED(*(const uint32_t *)b, ORC_SITE_BC6H_DUP_SKIP | ORC_SITE_BC6H_COMMIT_LOOP, out, 16, 16,
                  bc6h_encode_group(in, sitedOut, (const orc_options *)a, 0, rcp, sitedMask, siteLane));
}
static void bc6hs_group_thunk(const uint8_t *in, uint8_t *out, const void *a, const void *b, const float *rcp, size_t group)
{
    (void)group;
    ORC_RUN_SITED(*(const uint32_t *)b, ORC_SITE_BC6H_DUP_SKIP | ORC_SITE_BC6H_COMMIT_LOOP, out, 16, 16,
                  bc6h_encode_group(in, sitedOut, (const orc_options *)a, 1, rcp, sitedMask, siteLane));
}

int orc_encode_bc6h(uint8_t *out, const uint8_t *blocksF16, size_t numBlocks, const orc_options *options, int isSigned,
                    const float *rcp17, int threads)
{
    return orc_encode_bc6h_sites(out, blocksF16, numBlocks, options, isSigned, rcp17, threads, 0);
}

int orc_encode_bc6h_sites(uint8_t *out, const uint8_t *blocksF16, size_t numBlocks, const orc_options *options, int isSigned,
                          const float *rcp17, int threads, uint32_t siteMask)
{
    if (numBlocks % 8 != 0)
        return -1;
    float probed[17];
    if (!rcp17)
    {
        orc_probe_rcp(probed);
        rcp17 = probed;
    }
    run_groups(isSigned ? bc6hs_group_thunk : bc6hu_group_thunk, blocksF16, out, numBlocks / 8, 8 * 128, 8 * 16, options, &siteMask,
               rcp17, threads);
    return 0;
}
