/* TEST INFRASTRUCTURE ONLY -- BC1 (S3TCComputer::PackRGB, alpha-test variant) restatement.
 * Included by cvtt_oracle.c.  Follows ConvectionKernels_S3TC.cpp:52-304, 717-1052
 * (seeded search and S3TC_Exhaustive). */

/* QuantizeTo5Bits / QuantizeTo6Bits, S3TC.cpp:52-62 (16-bit wrapping) */
static int s3tc_quantize5(int v)
{
    uint16_t reduced = (uint16_t)((uint16_t)((uint16_t)((uint16_t)v * 249u) + 1024u) >> 11);
    return (uint16_t)((uint16_t)(reduced << 3) | (uint16_t)(reduced >> 2));
}

static int s3tc_quantize6(int v)
{
    uint16_t reduced = (uint16_t)((uint16_t)((uint16_t)((uint16_t)v * 253u) + 512u) >> 10);
    return (uint16_t)((uint16_t)(reduced << 2) | (uint16_t)(reduced >> 4));
}

typedef struct
{
    float bestError;
    int bestEndpoints[2][3];
    int bestIndexes[16];
    int bestRange;
} s3tc_best_t;

/* S3TCComputer::TestEndpoints, S3TC.cpp:190-258 */
static void s3tc_test_endpoints(uint32_t flags, const int pixels[16][4], const float floatPixels[16][4],
                                const float preWeighted[16][4], const int unquantized[2][4], int range,
                                const float *channelWeights, s3tc_best_t *best, refiner_t *refiner)
{
    float wSq[3];
    for (int ch = 0; ch < 3; ch++)
        wSq[ch] = channelWeights[ch] * channelWeights[ch];

    int endPoints[2][4];
    for (int ep = 0; ep < 2; ep++)
    {
        endPoints[ep][0] = s3tc_quantize5(unquantized[ep][0]);
        endPoints[ep][1] = s3tc_quantize6(unquantized[ep][1]);
        endPoints[ep][2] = s3tc_quantize5(unquantized[ep][2]);
        endPoints[ep][3] = 0;
    }

    selector_t sel;
    selector_init(&sel, 3, channelWeights, endPoints, range);

    float paranoidFactors[3];
    for (int ch = 0; ch < 3; ch++)
    {
        int16_t span = (int16_t)(endPoints[0][ch] - endPoints[1][ch]);
        paranoidFactors[ch] = fabsf((float)span) * 0.03f; /* ParanoidFactorForSpan, S3TC.cpp:71-74 */
    }

    int indexes[16];
    float error = 0.0f;
    aggerr_t agg;
    agg_init(&agg);
    for (int px = 0; px < 16; px++)
    {
        int index = selector_select(&sel, floatPixels[px]);
        indexes[px] = index;
        if (refiner)
            refiner_contribute_unweighted(refiner, preWeighted[px], index, 3);
        int rec[3];
        selector_reconstruct_precise(&sel, index, rec, 3);
        if (flags & ORC_FLAG_S3TC_PARANOID)
        {
            for (int ch = 0; ch < 3; ch++)
            {
                /* ParanoidDiff, S3TC.cpp:76-81 */
                float absDiff = fabsf((float)(int16_t)(rec[ch] - pixels[px][ch]));
                absDiff = absDiff + paranoidFactors[ch];
                error = error + absDiff * absDiff * wSq[ch];
            }
        }
        else
            agg_add_pixel(&agg, rec, pixels[px], 3);
    }
    if (!(flags & ORC_FLAG_S3TC_PARANOID))
        error = agg_finalize(&agg, 3, flags, wSq);

    if (error < best->bestError)
    {
        best->bestError = error;
        for (int ep = 0; ep < 2; ep++)
            for (int ch = 0; ch < 3; ch++)
                best->bestEndpoints[ep][ch] = endPoints[ep][ch];
        memcpy(best->bestIndexes, indexes, sizeof(indexes));
        best->bestRange = range;
    }
}

/* S3TCComputer::PackRGB for one block, S3TC.cpp:717-1052 (lanes are independent on the
 * non-exhaustive path: every AnySet there only guards per-lane conditional sets) */
typedef struct
{
    int pixels[16][4];
    float floatPixels[16][4], preWeighted[16][4];
    float w[4];
    unfinished_t ufep;
    s3tc_best_t best;
    int numRefineRounds, maxTweakRounds;
    /* exhaustive search only */
    int numElements;
    float pwSorted[16][4];
} s3tc_lane_t;

/* alphaTest: 1 = BC1 (EncodeBC1), 0 = the colour half of BC2 / BC3 (API.cpp:101-130) */
static void s3tc_prepare(s3tc_lane_t *ln, const uint8_t *block, const orc_options *options, int alphaTest)
{
    float *w = ln->w;
    fill_weights(options, w);
    int numRefineRounds = options->refineRoundsS3TC;
    int maxTweakRounds = options->seedPoints;
    if (numRefineRounds < 1) numRefineRounds = 1;
    if (maxTweakRounds < 1) maxTweakRounds = 1;
    ln->numRefineRounds = numRefineRounds;
    ln->maxTweakRounds = maxTweakRounds;
    int (*pixels)[4] = ln->pixels;
    float (*floatPixels)[4] = ln->floatPixels, (*preWeighted)[4] = ln->preWeighted;
    unfinished_t ufep;
    for (int px = 0; px < 16; px++)
        for (int ch = 0; ch < 4; ch++)
        {
            pixels[px][ch] = block[px * 4 + ch];
            floatPixels[px][ch] = (float)pixels[px][ch]; /* taken BEFORE the alpha threshold, S3TC.cpp:740-755 */
        }
    /* alpha test, S3TC.cpp:746-755 */
    if (alphaTest)
    {
        const int threshold = (uint16_t)floor(options->threshold * 255.0f + 0.5f);
        for (int px = 0; px < 16; px++)
            pixels[px][3] = ((int16_t)pixels[px][3] < (int16_t)threshold) ? 0 : 255;
    }
    for (int px = 0; px < 16; px++)
        for (int ch = 0; ch < 4; ch++)
            preWeighted[px][ch] = (float)pixels[px][ch] * w[ch];

    /* weighted PCA: transparent pixels have weight 0 in passes 0/1 but still take part in the
     * min/max pass (EndpointSelector.h:33-48, 132-140; S3TC.cpp:764-782) */
    {
        uint8_t opaque[16];
        int nOpaque = 0;
        for (int px = 0; px < 16; px++)
            if (!(pixels[px][3] < 255))
                opaque[nOpaque++] = (uint8_t)px;
        /* passes 0 and 1 over the weighted (= opaque) pixels, pass 2 over all 16: reuse
         * pca_endpoints twice is not possible (pass 2 depends on pass 0/1), so inline it */
        float centroid[3] = {0, 0, 0}, cov[6] = {0, 0, 0, 0, 0, 0}, weightTotal = 0.0f;
        for (int px = 0; px < 16; px++)
        {
            float weight = (alphaTest && pixels[px][3] < 255) ? 0.0f : 1.0f;
            for (int ch = 0; ch < 3; ch++)
                centroid[ch] = centroid[ch] + preWeighted[px][ch] * weight;
            weightTotal = weightTotal + weight;
        }
        float denom = f_safe_denom(weightTotal);
        for (int ch = 0; ch < 3; ch++)
            centroid[ch] = centroid[ch] / denom;
        for (int px = 0; px < 16; px++)
        {
            float weight = (alphaTest && pixels[px][3] < 255) ? 0.0f : 1.0f;
            float diff[3];
            for (int ch = 0; ch < 3; ch++)
                diff[ch] = preWeighted[px][ch] - centroid[ch];
            int index = 0;
            for (int row = 0; row < 3; row++)
                for (int col = 0; col <= row; col++)
                {
                    cov[index] = cov[index] + diff[row] * diff[col] * weight;
                    index++;
                }
        }
        float approx[3] = {1.0f, 1.0f, 1.0f};
        for (int it = 0; it < 8; it++)
        {
            float product[3];
            for (int row = 0; row < 3; row++)
            {
                float sum = 0.0f;
                int index = (row * (row + 1)) >> 1;
                for (int col = 0; col < 3; col++)
                {
                    sum = sum + approx[col] * cov[index];
                    if (col >= row) index += col + 1; else index++;
                }
                product[row] = sum;
            }
            float largest = product[0];
            for (int ch = 1; ch < 3; ch++)
                largest = f_max(largest, product[ch]);
            largest = f_safe_denom(largest);
            for (int ch = 0; ch < 3; ch++)
                approx[ch] = product[ch] / largest;
        }
        float approxLen = 0.0f;
        for (int ch = 0; ch < 3; ch++)
            approxLen = approxLen + approx[ch] * approx[ch];
        approxLen = f_safe_denom(sqrtf(approxLen));
        float direction[3];
        for (int ch = 0; ch < 3; ch++)
            direction[ch] = approx[ch] / approxLen;
        float minDist = FLT_MAX, maxDist = -FLT_MAX;
        for (int px = 0; px < 16; px++)
        {
            float dist = 0.0f;
            for (int ch = 0; ch < 3; ch++)
                dist = dist + direction[ch] * (preWeighted[px][ch] - centroid[ch]);
            minDist = f_min(minDist, dist);
            maxDist = f_max(maxDist, dist);
        }
        for (int ch = 0; ch < 3; ch++)
        {
            float mn = centroid[ch] + direction[ch] * minDist;
            float mx = centroid[ch] + direction[ch] * maxDist;
            ufep.base[ch] = mn / w[ch];
            ufep.offset[ch] = (mx - mn) / w[ch];
        }
        ufep.base[3] = ufep.offset[3] = 0.0f;
        (void)opaque;
    }

    ln->ufep = ufep;
    memset(&ln->best, 0, sizeof(ln->best));
    ln->best.bestError = FLT_MAX;
}

/* the non-exhaustive search, S3TC.cpp:937-965 */
static void s3tc_search(s3tc_lane_t *ln, uint32_t flags, const float *rcp, int alphaTest)
{
    const float *w = ln->w;
    const int numRefineRounds = ln->numRefineRounds, maxTweakRounds = ln->maxTweakRounds;
    int (*pixels)[4] = ln->pixels;
    float (*floatPixels)[4] = ln->floatPixels, (*preWeighted)[4] = ln->preWeighted;
    unfinished_t ufep = ln->ufep;
    s3tc_best_t best = ln->best;

    /* ranges 3 and 4 with the alpha test (BC1), range 4 only without, S3TC.cpp:937-965 */
    for (int range = alphaTest ? 3 : 4; range <= 4; range++)
    {
        int tweakRounds = (range == 3) ? 3 : 4; /* BCCommon::TweakRoundsForRange */
        if (tweakRounds > maxTweakRounds)
            tweakRounds = maxTweakRounds;
        for (int tweak = 0; tweak < tweakRounds; tweak++)
        {
            int endPoints[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            finish_ldr(&ufep, 3, tweak, range, endPoints[0], endPoints[1]);
            for (int refine = 0; refine < numRefineRounds; refine++)
            {
                refiner_t refiner;
                refiner_init(&refiner, 3, range, w, rcp);
                s3tc_test_endpoints(flags, pixels, floatPixels, preWeighted, endPoints, range, w, &best, &refiner);
                if (refine != numRefineRounds - 1)
                    refiner_get_ldr(&refiner, endPoints);
            }
        }
    }

    ln->best = best;
}

/* colour ordering + index remap + bytes, S3TC.cpp:967-1051 */
static void s3tc_emit(const s3tc_lane_t *ln, uint8_t *out)
{
    const s3tc_best_t best = ln->best;
    /* colour ordering + index remap, S3TC.cpp:967-1051 */
    const int range = best.bestRange;
    unsigned compressedEP[2];
    for (int ep = 0; ep < 2; ep++)
    {
        unsigned c = (unsigned)(best.bestEndpoints[ep][0] & 0xf8) << 8;
        c |= (unsigned)(best.bestEndpoints[ep][1] & 0xfc) << 3;
        c |= (unsigned)(best.bestEndpoints[ep][2] & 0xf8) >> 3;
        compressedEP[ep] = c & 0xffffu;
    }
    int indexOrder[4];
    if (range == 4)
    {
        if (compressedEP[0] == compressedEP[1])
            indexOrder[0] = indexOrder[1] = indexOrder[2] = indexOrder[3] = 0;
        else if (compressedEP[0] < compressedEP[1])
        {
            unsigned t = compressedEP[0]; compressedEP[0] = compressedEP[1]; compressedEP[1] = t;
            indexOrder[0] = 1; indexOrder[1] = 3; indexOrder[2] = 2; indexOrder[3] = 0;
        }
        else
        {
            indexOrder[0] = 0; indexOrder[1] = 2; indexOrder[2] = 3; indexOrder[3] = 1;
        }
    }
    else
    {
        if (compressedEP[0] > compressedEP[1])
        {
            unsigned t = compressedEP[0]; compressedEP[0] = compressedEP[1]; compressedEP[1] = t;
            indexOrder[0] = 1; indexOrder[1] = 2; indexOrder[2] = 0;
        }
        else
        {
            indexOrder[0] = 0; indexOrder[1] = 2; indexOrder[2] = 1;
        }
        indexOrder[3] = 3;
    }
    out[0] = (uint8_t)(compressedEP[0] & 0xff);
    out[1] = (uint8_t)((compressedEP[0] >> 8) & 0xff);
    out[2] = (uint8_t)(compressedEP[1] & 0xff);
    out[3] = (uint8_t)((compressedEP[1] >> 8) & 0xff);
    for (int i = 0; i < 16; i += 4)
    {
        int packed = 0;
        for (int subi = 0; subi < 4; subi++)
            packed |= indexOrder[best.bestIndexes[i + subi] & 3] << (subi * 2);
        out[4 + i / 4] = (uint8_t)packed;
    }
}

/* ---- S3TC_Exhaustive: S3TC.cpp:798-936 (cluster-size enumeration over the pixels sorted along the PCA axis),
 * TestCounts 260-304, TestSingleColor 83-188.  The 8 lanes of a group are coupled through TestCounts' escape
 * (AnySet(valid), S3TC.cpp:275-281): contributions stop for everybody where no lane has elements left. ---- */
static void s3tc_test_single_color(s3tc_lane_t *ln, uint32_t flags, int range)
{
    float wSq[3];
    for (int ch = 0; ch < 3; ch++)
        wSq[ch] = ln->w[ch] * ln->w[ch];
    int average[3];
    for (int ch = 0; ch < 3; ch++)
    {
        uint16_t total = 0;
        for (int px = 0; px < 16; px++)
            total = (uint16_t)(total + ln->pixels[px][ch]);
        average[ch] = (uint16_t)(total + 8) >> 4;
    }
    const int paranoid = (flags & ORC_FLAG_S3TC_PARANOID) != 0;
    const int t = (paranoid ? 4 : 0) + (range == 3 ? 2 : 0);
    int eps[2][3], interpolated[3], spans[3];
    for (int ch = 0; ch < 3; ch++)
    {
        const unsigned char *e = orc_s3tcsc[t + (ch == 1)][average[ch] & 255];
        eps[0][ch] = e[0];
        eps[1][ch] = e[1];
        interpolated[ch] = e[2];
        spans[ch] = e[3];
    }
    float error = 0.0f;
    for (int px = 0; px < 16; px++)
        for (int ch = 0; ch < 3; ch++)
        {
            if (paranoid)
            {
                float absDiff = fabsf((float)(int16_t)(interpolated[ch] - ln->pixels[px][ch]));
                absDiff = absDiff + fabsf((float)spans[ch]) * 0.03f;
                error = error + absDiff * absDiff * wSq[ch];
            }
            else
            {
                uint16_t d = (uint16_t)(interpolated[ch] - ln->pixels[px][ch]);
                error = error + (float)(uint16_t)(d * d) * wSq[ch];
            }
        }
    if (error < ln->best.bestError)
    {
        ln->best.bestError = error;
        for (int e = 0; e < 2; e++)
            for (int ch = 0; ch < 3; ch++)
                ln->best.bestEndpoints[e][ch] = eps[e][ch];
        for (int px = 0; px < 16; px++)
            ln->best.bestIndexes[px] = 1;
        ln->best.bestRange = range;
    }
}

static void s3tc_test_counts(s3tc_lane_t *lanes, uint32_t flags, const int *counts, int nCounts, int groupMaxElements, const float *rcp)
{
    for (int l = 0; l < 8; l++)
    {
        s3tc_lane_t *ln = &lanes[l];
        refiner_t refiner;
        refiner_init(&refiner, 3, nCounts, ln->w, rcp);
        int escape = 0, e = 0;
        for (int i = 0; i < nCounts && !escape; i++)
            for (int n = 0; n < counts[i]; n++)
            {
                if (!(n < groupMaxElements))
                {
                    escape = 1;
                    break;
                }
                if (n < ln->numElements)
                    refiner_contribute_unweighted(&refiner, ln->pwSorted[e], i, 3);
                e++;
            }
        int endPoints[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        refiner_get_ldr(&refiner, endPoints);
        s3tc_test_endpoints(flags, ln->pixels, ln->floatPixels, ln->preWeighted, endPoints, nCounts, ln->w, &ln->best, NULL);
    }
}

static void s3tc_exhaustive_group(s3tc_lane_t *lanes, uint32_t flags, const float *rcp, int alphaTest, uint32_t siteMask, int siteLane)
{
    int groupMaxElements = 0;
    for (int l = 0; l < 8; l++)
    {
        s3tc_lane_t *ln = &lanes[l];
        int sortEP[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        finish_ldr(&ln->ufep, 3, 0, 11, sortEP[0], sortEP[1]);
        selector_t sel;
        selector_init(&sel, 3, ln->w, sortEP, 1 << 11);
        int16_t bins[16];
        for (int px = 0; px < 16; px++)
        {
            int16_t bin = (int16_t)(selector_select(&sel, ln->floatPixels[px]) << 4);
            if (alphaTest && ln->pixels[px][3] < 255)
                bin = -16;
            bins[px] = (int16_t)(bin + px);
        }
        for (int sortEnd = 1; sortEnd < 16; sortEnd++)
            for (int loc = sortEnd; loc > 0; loc--)
            {
                int16_t a = bins[loc], b = bins[loc - 1];
                bins[loc] = a > b ? a : b;
                bins[loc - 1] = a > b ? b : a;
            }
        int firstElement = 0;
        for (int e = 0; e < 16; e++)
            if (bins[e] < 0)
                firstElement = e + 1;
        ln->numElements = 16 - firstElement;
        if (ln->numElements > groupMaxElements)
            groupMaxElements = ln->numElements;
        memset(ln->pwSorted, 0, sizeof(ln->pwSorted));
        for (int e = firstElement; e < 16; e++)
        {
            const int original = bins[e] & 15;
            for (int ch = 0; ch < 4; ch++)
                ln->pwSorted[15 - e][ch] = (float)ln->pixels[original][ch] * ln->w[ch];
        }
    }
    /* site switch: TestCounts' escape tests the viewing lane's own element count, not the group's largest */
    if (siteMask & ORC_SITE_BC1_TEST_COUNTS)
        groupMaxElements = lanes[siteLane].numElements;
    for (int n0 = 0; n0 <= 15; n0++)
    {
        int remainingFor1 = 16 - n0;
        if (remainingFor1 == 16) remainingFor1 = 15;
        for (int n1 = 0; n1 <= remainingFor1; n1++)
        {
            int remainingFor2 = 16 - n1 - n0;
            if (remainingFor2 == 16) remainingFor2 = 15;
            for (int n2 = 0; n2 <= remainingFor2; n2++)
            {
                const int n3 = 16 - n2 - n1 - n0;
                if (n3 == 16)
                    continue;
                const int counts[4] = {n0, n1, n2, n3};
                s3tc_test_counts(lanes, flags, counts, 4, groupMaxElements, rcp);
            }
        }
    }
    for (int l = 0; l < 8; l++)
        s3tc_test_single_color(&lanes[l], flags, 4);
    if (alphaTest)
    {
        for (int n0 = 0; n0 <= 15; n0++)
        {
            int remainingFor1 = 16 - n0;
            if (remainingFor1 == 16) remainingFor1 = 15;
            for (int n1 = 0; n1 <= remainingFor1; n1++)
            {
                const int n2 = 16 - n1 - n0;
                if (n2 == 16)
                    continue;
                const int counts[3] = {n0, n1, n2};
                s3tc_test_counts(lanes, flags, counts, 3, groupMaxElements, rcp);
            }
        }
        for (int l = 0; l < 8; l++)
            s3tc_test_single_color(&lanes[l], flags, 3);
    }
}

/* PackRGB for a group of 8 blocks (outputs `stride` apart).  err: NULL, or 8 floats that receive each block's final
 * bestError, the score of the candidate that is emitted. */
static void s3tc_pack_rgb_group(const uint8_t *blocks, uint8_t *out, size_t stride, const orc_options *options, const float *rcp, int alphaTest,
                                float *err, uint32_t siteMask, int siteLane)
{
    static __thread s3tc_lane_t lanes[8];
    for (int l = 0; l < 8; l++)
        s3tc_prepare(&lanes[l], blocks + l * 64, options, alphaTest);
    if (options->flags & ORC_FLAG_S3TC_EXHAUSTIVE)
        s3tc_exhaustive_group(lanes, options->flags, rcp, alphaTest, siteMask, siteLane);
    else
        for (int l = 0; l < 8; l++)
            s3tc_search(&lanes[l], options->flags, rcp, alphaTest);
    for (int l = 0; l < 8; l++)
        s3tc_emit(&lanes[l], out + l * stride);
    if (err)
        for (int l = 0; l < 8; l++)
            err[l] = lanes[l].best.bestError;
}

static void s3tc_pack_rgb(const uint8_t *block, uint8_t *out, const orc_options *options, const float *rcp, int alphaTest)
{
    s3tc_lane_t ln;
    s3tc_prepare(&ln, block, options, alphaTest);
    s3tc_search(&ln, options->flags, rcp, alphaTest);
    s3tc_emit(&ln, out);
}

typedef struct { const orc_options *options; float *err; /* NULL, or one float per block */ uint32_t siteMask; } bc1_job_t;

static void bc1_group_thunk(const uint8_t *in, uint8_t *out, const void *a, const void *b, const float *rcp, size_t group)
{
    (void)b;
    const bc1_job_t *job = (const bc1_job_t *)a;
    float *err = job->err ? job->err + group * 8 : NULL;
    ORC_RUN_SITED(job->siteMask, ORC_SITE_BC1_TEST_COUNTS, out, 8, 8,
                  s3tc_pack_rgb_group(in, sitedOut, 8, job->options, rcp, 1, sitedMask ? NULL : err, sitedMask, siteLane));
}

static int bc1_encode(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                      const float *rcp17, int threads, float *err, uint32_t siteMask)
{
    if (numBlocks % 8 != 0)
        return -1;
    float probed[17];
    if (!rcp17)
    {
        orc_probe_rcp(probed);
        rcp17 = probed;
    }
    bc1_job_t job = {options, err, siteMask};
    run_groups(bc1_group_thunk, blocks, out, numBlocks / 8, 8 * 64, 8 * 8, &job, NULL, rcp17, threads);
    return 0;
}

int orc_encode_bc1(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                   const float *rcp17, int threads)
{
    return bc1_encode(out, blocks, numBlocks, options, rcp17, threads, NULL, 0);
}

int orc_encode_bc1_sites(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                         const float *rcp17, int threads, uint32_t siteMask)
{
    return bc1_encode(out, blocks, numBlocks, options, rcp17, threads, NULL, siteMask);
}
