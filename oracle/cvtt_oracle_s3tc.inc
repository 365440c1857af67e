/* TEST INFRASTRUCTURE ONLY -- BC2 / BC3 / BC4 / BC5 restatement, included by cvtt_oracle.c.
 * PackInterpolatedAlpha, S3TC.cpp:343-715; PackExplicitAlpha, S3TC.cpp:306-341; entry points API.cpp:101-199.
 * Lanes are independent: every AnySet / AllSet on this path only skips work that cannot change a lane (duplicate
 * end-point pairs re-evaluated under a strict '<'; ContributePW with weight 1.0 equals ContributeUnweightedPW, and
 * m_w + m_wu is the lane's own contribution count either way, EndpointRefiner.h:62-104). */

/* ParallelMath::LessOrEqual(UInt15) is implemented as '<' (ParallelMath.h:740-745); only this path uses it */
static inline int s3tc_le_u15(int a, int b) { return a < b; }

/* errOut: NULL, or where the final bestError (the score of the emitted end points and indexes) goes */
static void s3tc_interpolated_alpha(const uint8_t *block, int inputChannel, uint8_t *out, uint32_t flags, int isSigned,
                                    int maxTweakRounds, int numRefineRounds, const float *rcp, float *errOut)
{
    (void)flags;
    if (maxTweakRounds < 1) maxTweakRounds = 1;
    if (numRefineRounds < 1) numRefineRounds = 1;
    const float oneWeight[1] = {1.0f};
    const int highTerminal = isSigned ? 254 : 255;
    int pixels[16], sorted[16];
    float floatPixels[16];
    for (int px = 0; px < 16; px++)
    {
        int v = block[px * 4 + inputChannel];
        if (isSigned && v > highTerminal) v = highTerminal;
        pixels[px] = v;
        floatPixels[px] = (float)v;
        sorted[px] = v;
    }
    for (int sortEnd = 15; sortEnd > 0; sortEnd--)
        for (int o = 0; o < sortEnd; o++)
        {
            int a = sorted[o], b = sorted[o + 1];
            sorted[o] = a < b ? a : b;
            sorted[o + 1] = a < b ? b : a;
        }

    int bestIsFullRange = 0, bestEP[2] = {0, 0}, bestIndexes[16];
    float bestError = FLT_MAX;
    memset(bestIndexes, 0, sizeof(bestIndexes));

    /* full precision: 8 interpolated values */
    {
        unfinished_t ufep;
        memset(&ufep, 0, sizeof(ufep));
        ufep.base[0] = (float)sorted[0];
        ufep.offset[0] = (float)(sorted[15] - sorted[0]);
        int numTweakRounds = 4; /* TweakRoundsForRange(8) */
        if (numTweakRounds > maxTweakRounds) numTweakRounds = maxTweakRounds;
        for (int tweak = 0; tweak < numTweakRounds; tweak++)
        {
            int ep[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            finish_ldr(&ufep, 1, tweak, 8, ep[0], ep[1]);
            for (int refinePass = 0; refinePass < numRefineRounds; refinePass++)
            {
                refiner_t refiner;
                refiner_init(&refiner, 1, 8, oneWeight, rcp);
                if (isSigned)
                    for (int e = 0; e < 2; e++)
                        if (ep[e][0] > highTerminal) ep[e][0] = highTerminal;
                selector_t sel;
                selector_init(&sel, 1, oneWeight, ep, 8);
                int indexes[16];
                uint32_t agg = 0;
                for (int px = 0; px < 16; px++)
                {
                    int index = selector_select(&sel, &floatPixels[px]);
                    int rec[1];
                    selector_reconstruct_precise(&sel, index, rec, 1);
                    uint16_t d = (uint16_t)(rec[0] - pixels[px]);
                    agg += (uint16_t)(d * d);
                    if (refinePass != numRefineRounds - 1)
                        refiner_contribute_unweighted(&refiner, &floatPixels[px], index, 1);
                    indexes[px] = index;
                }
                const float error = (float)(int32_t)agg; /* Finalize(flags | Uniform) */
                if (error < bestError)
                {
                    bestError = error;
                    bestIsFullRange = 1;
                    memcpy(bestIndexes, indexes, sizeof(indexes));
                    bestEP[0] = ep[0][0];
                    bestEP[1] = ep[1][0];
                }
                if (refinePass != numRefineRounds - 1)
                    refiner_get_ldr(&refiner, ep);
            }
        }
    }

    /* reduced precision: 6 interpolated values + the terminals 0 and highTerminal */
    {
        int bestHeuristicMin = sorted[0], bestHeuristicMax = sorted[15];
        int canTryClipping;
        {
            int largestPossibleRange = (uint16_t)(bestHeuristicMax - bestHeuristicMin);
            int hiClear = (uint16_t)(highTerminal - bestHeuristicMax);
            int lowestPossibleClearance = bestHeuristicMin < hiClear ? bestHeuristicMin : hiClear;
            int times10 = (uint16_t)((lowestPossibleClearance << 2) + (lowestPossibleClearance << 4));
            canTryClipping = s3tc_le_u15(times10, largestPossibleRange);
        }
        if (canTryClipping)
        {
            int lowClearances[16], highClearances[16], bestSkipCount = 0;
            lowClearances[0] = highClearances[0] = 0;
            for (int px = 1; px < 16; px++)
            {
                lowClearances[px] = sorted[px - 1];
                highClearances[px] = (uint16_t)(highTerminal - sorted[16 - px]);
            }
            for (int firstIndex = 0; firstIndex < 16; firstIndex++)
            {
                const int numSkippedLow = firstIndex, lowClearance = lowClearances[firstIndex];
                for (int lastIndex = firstIndex; lastIndex < 16; lastIndex++)
                {
                    const int numSkippedHigh = 15 - lastIndex, numSkipped = numSkippedLow + numSkippedHigh;
                    if (!(bestSkipCount < numSkipped))
                        continue;
                    int clearance = highClearances[numSkippedHigh] > lowClearance ? highClearances[numSkippedHigh] : lowClearance;
                    int times10 = (uint16_t)((clearance << 2) + (clearance << 4));
                    int range = (uint16_t)(sorted[lastIndex] - sorted[firstIndex]);
                    if (s3tc_le_u15(times10, range))
                    {
                        /* NB: bestSkipCount is never updated by the reference (S3TC.cpp:497-527) */
                        bestHeuristicMin = sorted[firstIndex];
                        bestHeuristicMax = sorted[lastIndex];
                    }
                }
            }
        }
        int bestSimpleMin = 1, bestSimpleMax = highTerminal - 1;
        for (int px = 0; px < 16; px++)
        {
            if (0 < sorted[15 - px]) bestSimpleMin = sorted[15 - px];
            if (sorted[px] < highTerminal) bestSimpleMax = sorted[px];
        }
        const int minEPs[2] = {bestSimpleMin, bestHeuristicMin}, maxEPs[2] = {bestSimpleMax, bestHeuristicMax};
        for (int minEPIndex = 0; minEPIndex < 2; minEPIndex++)
            for (int maxEPIndex = 0; maxEPIndex < 2; maxEPIndex++)
            {
                unfinished_t ufep;
                memset(&ufep, 0, sizeof(ufep));
                ufep.base[0] = (float)minEPs[minEPIndex];
                ufep.offset[0] = (float)(uint16_t)(maxEPs[maxEPIndex] - minEPs[minEPIndex]);
                int numTweakRounds = 4; /* TweakRoundsForRange(6) */
                if (numTweakRounds > maxTweakRounds) numTweakRounds = maxTweakRounds;
                for (int tweak = 0; tweak < numTweakRounds; tweak++)
                {
                    int ep[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
                    finish_ldr(&ufep, 1, tweak, 8, ep[0], ep[1]);
                    for (int refinePass = 0; refinePass < numRefineRounds; refinePass++)
                    {
                        refiner_t refiner;
                        refiner_init(&refiner, 1, 6, oneWeight, rcp);
                        if (isSigned)
                            for (int e = 0; e < 2; e++)
                                if (ep[e][0] > highTerminal) ep[e][0] = highTerminal;
                        selector_t sel;
                        selector_init(&sel, 1, oneWeight, ep, 6);
                        int indexes[16];
                        float error = 0.0f;
                        for (int px = 0; px < 16; px++)
                        {
                            int selectedIndex = selector_select(&sel, &floatPixels[px]);
                            int rec[1];
                            selector_reconstruct_precise(&sel, selectedIndex, rec, 1);
                            uint16_t d0 = (uint16_t)(0 - pixels[px]), dh = (uint16_t)(highTerminal - pixels[px]), ds = (uint16_t)(rec[0] - pixels[px]);
                            float zeroError = (float)(int32_t)(uint32_t)(uint16_t)(d0 * d0);
                            float highTerminalError = (float)(int32_t)(uint32_t)(uint16_t)(dh * dh);
                            float selectedIndexError = (float)(int32_t)(uint32_t)(uint16_t)(ds * ds);
                            float bestPixelError = zeroError;
                            int index = 6;
                            if (highTerminalError < bestPixelError) index = 7;
                            bestPixelError = f_min(bestPixelError, highTerminalError);
                            const int selectedIndexBetter = selectedIndexError < bestPixelError;
                            if (refinePass != numRefineRounds - 1 && selectedIndexBetter)
                                refiner_contribute_unweighted(&refiner, &floatPixels[px], selectedIndex, 1);
                            if (selectedIndexBetter) index = selectedIndex;
                            bestPixelError = f_min(bestPixelError, selectedIndexError);
                            error = error + bestPixelError;
                            indexes[px] = index;
                        }
                        if (error < bestError)
                        {
                            bestError = error;
                            bestIsFullRange = 0;
                            memcpy(bestIndexes, indexes, sizeof(indexes));
                            bestEP[0] = ep[0][0];
                            bestEP[1] = ep[1][0];
                        }
                        if (refinePass != numRefineRounds - 1)
                            refiner_get_ldr(&refiner, ep);
                    }
                }
            }
    }

    if (errOut)
        *errOut = bestError;
    int ep0 = bestEP[0], ep1 = bestEP[1];
    if (isSigned)
    {
        ep0 -= 127;
        ep1 -= 127;
    }
    const int swapEndpoints = (bestIsFullRange != 0) != (ep0 > ep1);
    if (swapEndpoints)
    {
        int t = ep0; ep0 = ep1; ep1 = t;
    }
    out[0] = (uint8_t)(ep0 & 0xff);
    out[1] = (uint8_t)(ep1 & 0xff);
    const int maxValue = bestIsFullRange ? 7 : 5;
    unsigned dumpBits = 0;
    int dumpBitsOffset = 0, dumpByteOffset = 2;
    for (int px = 0; px < 16; px++)
    {
        int index = bestIndexes[px];
        if (swapEndpoints && index <= maxValue) index = maxValue - index;
        if (index != 0)
        {
            if (index == maxValue) index = 1;
            else if (index < maxValue) index++;
        }
        dumpBits |= (unsigned)(index << dumpBitsOffset) & 0xffffu;
        dumpBitsOffset += 3;
        if (dumpBitsOffset >= 8)
        {
            out[dumpByteOffset++] = (uint8_t)(dumpBits & 0xff);
            dumpBits >>= 8;
            dumpBitsOffset -= 8;
        }
    }
}

static void s3tc_explicit_alpha(const uint8_t *block, int inputChannel, uint8_t *out)
{
    const float oneWeight[1] = {1.0f};
    int ep[2][4] = {{0, 0, 0, 0}, {255, 0, 0, 0}};
    selector_t sel;
    selector_init(&sel, 1, oneWeight, ep, 16);
    for (int px = 0; px < 16; px += 2)
    {
        float f0 = (float)block[px * 4 + inputChannel], f1 = (float)block[(px + 1) * 4 + inputChannel];
        int i0 = selector_select(&sel, &f0), i1 = selector_select(&sel, &f1);
        out[px / 2] = (uint8_t)(i0 | (i1 << 4));
    }
}

/* format: 2 = BC2, 3 = BC3, 4 = BC4U, 5 = BC4S, 6 = BC5U, 7 = BC5S.  Signed formats take PixelBlockS8 (biased like
 * Util::BiasSignedInput, Util.cpp:47-60).  Output 8 bytes (BC4) or 16 bytes per block. */
typedef struct
{
    const orc_options *options;
    int format;
    float *colorErr; /* NULL, or one float per block (BC2, BC3) */
    float *alphaErr; /* NULL, or one float per block and interpolated channel (BC3, BC4: 1; BC5: 2) */
} s3tc_job_t;

static void s3tc_group_thunk(const uint8_t *in, uint8_t *out, const void *a, const void *b, const float *rcp, size_t group)
{
    (void)b;
    const s3tc_job_t *job = (const s3tc_job_t *)a;
    const orc_options *o = job->options;
    if (job->format == 2 || job->format == 3)
        s3tc_pack_rgb_group(in, out + 8, 16, o, rcp, 0, job->colorErr ? job->colorErr + group * 8 : NULL, 0, 0);
    const int alphaChannels = job->format >= 6 ? 2 : 1;
    for (int blk = 0; blk < 8; blk++)
    {
        float *aerr = job->alphaErr ? job->alphaErr + (group * 8 + (size_t)blk) * (size_t)alphaChannels : NULL;
        const uint8_t *src = in + blk * 64;
        uint8_t biased[64];
        if (job->format == 5 || job->format == 7)
        {
            for (int i = 0; i < 64; i++)
            {
                int v = (int8_t)src[i];
                biased[i] = (uint8_t)((v < -127 ? -127 : v) + 127);
            }
            src = biased;
        }
        switch (job->format)
        {
        case 2:
            s3tc_explicit_alpha(src, 3, out + blk * 16);
            break;
        case 3:
            s3tc_interpolated_alpha(src, 3, out + blk * 16, o->flags, 0, o->seedPoints, o->refineRoundsIIC, rcp, aerr);
            break;
        case 4:
        case 5:
            s3tc_interpolated_alpha(src, 0, out + blk * 8, o->flags, job->format == 5, o->seedPoints, o->refineRoundsIIC, rcp, aerr);
            break;
        default:
            s3tc_interpolated_alpha(src, 0, out + blk * 16, o->flags, job->format == 7, o->seedPoints, o->refineRoundsIIC, rcp, aerr);
            s3tc_interpolated_alpha(src, 1, out + blk * 16 + 8, o->flags, job->format == 7, o->seedPoints, o->refineRoundsIIC, rcp,
                                    aerr ? aerr + 1 : NULL);
            break;
        }
    }
}

static int s3tc_encode(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, int format,
                       const float *rcp17, int threads, float *colorErr, float *alphaErr)
{
    if (numBlocks % 8 != 0 || format < 2 || format > 7)
        return -1;
    float probed[17];
    if (!rcp17)
    {
        orc_probe_rcp(probed);
        rcp17 = probed;
    }
    s3tc_job_t job = {options, format, colorErr, format == 2 ? NULL : alphaErr};
    const size_t outPer = (format == 4 || format == 5) ? 8 : 16;
    run_groups(s3tc_group_thunk, blocks, out, numBlocks / 8, 8 * 64, 8 * outPer, &job, NULL, rcp17, threads);
    return 0;
}

int orc_encode_s3tc(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, int format,
                    const float *rcp17, int threads)
{
    return s3tc_encode(out, blocks, numBlocks, options, format, rcp17, threads, NULL, NULL);
}
