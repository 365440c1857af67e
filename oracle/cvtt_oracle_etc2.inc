/* TEST INFRASTRUCTURE ONLY -- ETC2 RGB / RGBA / EAC-alpha restatement, included by cvtt_oracle.c.
 * Follows ConvectionKernels_ETC.cpp: ExtractBlocks 2128-2155, EncodePlanar 1266-1662,
 * sector split 1723-1848, EncodeTMode 396-647, EncodeHMode 649-885, CompressETC1BlockInternal
 * 2624-2882 (differential only: ETC2 calls it with punchthrough = true, ETC.cpp:1862, 2677),
 * TestHalfBlock 94-149, FindBestDifferentialCombination 219-362, emitters 2414-2622,
 * CompressETC2AlphaBlockInternal 1902-2085, QuantizeETC2Alpha 2366-2411, chroma axes 3117-3145.
 * Canonical oracle semantics (SURVEY App. C): hazard H2 -- the T-mode candidate slot just past a
 * lane's unique colours reads as 0 when another lane of the group has more unique colours.
 * ETC_UseFakeBT709 and ETC_FakeBT709Accurate are restated too (etc_ctx_t.fake / fakeAccurate). */
#include "cvtt_oracle_etc_tables.h"
#include "cvtt_oracle_fake709.h"

typedef struct
{
    uint32_t flags;
    int uniform;
    float rw, gw, bw;       /* weights straight from Options (ETC.cpp:2150-2152) */
    float axis0[3], axis1[3];
    int fake;               /* ETC_UseFakeBT709: errors in a luma/chroma space (ETC.cpp:82-92, 2329-2364) */
    int fakeAccurate;       /* ETC_FakeBT709Accurate: octant search instead of the rounding table (ETC.cpp:2757-2760) */
    int punchthrough;       /* EncodeETC2PunchthroughAlpha */
    int alphaThreshold;     /* floor(clamp(threshold, 0, 1) * 255 + 1), ETC.cpp:1672-1675 */
} etc_ctx_t;

typedef struct
{
    int pixels[16][3];
    float pw[16][3];
    float bestError;
    uint8_t out[8];
    int isolated[16];    /* sector assignment of the first T-mode call */
    int tUnique[2][8];   /* unique line colours per T-mode call and table */
    int transparent[16]; /* punch-through: alpha below the threshold (ETC.cpp:1670-1688) */
    int anyTransparent, allTransparent, numOpaque;
} etc_lane_t;

/* ETC2CompressionDataInternal constructor, ETC.cpp:3117-3145 */
static void etc2_chroma_axes(const orc_options *o, float axis0[3], float axis1[3])
{
    const float cd[3] = {o->redWeight, o->greenWeight, o->blueWeight};
    const float rotCD[3] = {cd[1], cd[2], cd[0]};
    const float offs = -(rotCD[0] * cd[0] + rotCD[1] * cd[1] + rotCD[2] * cd[2]) / (cd[0] * cd[0] + cd[1] * cd[1] + cd[2] * cd[2]);
    const float a0[3] = {rotCD[0] + cd[0] * offs, rotCD[1] + cd[1] * offs, rotCD[2] + cd[2] * offs};
    const float a1u[3] = {a0[1] * cd[2] - a0[2] * cd[1], a0[2] * cd[0] - a0[0] * cd[2], a0[0] * cd[1] - a0[1] * cd[0]};
    const float l0 = (a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]);
    const float l1 = (a1u[0] * a1u[0] + a1u[1] * a1u[1] + a1u[2] * a1u[2]);
    const float ratio = (float)sqrt((double)(l0 / l1));
    for (int i = 0; i < 3; i++)
    {
        axis0[i] = a0[i];
        axis1[i] = a1u[i] * ratio;
    }
}

/* ConvertToFakeBT709, ETC.cpp:2343-2352 */
static inline void etc_to_fake709(float yuv[3], float r, float g, float b)
{
    yuv[0] = r * 0.368233989135369f + g * 1.23876274963149f + b * 0.125054068802017f;
    yuv[1] = r * 0.5f - g * 0.4541529f - b * 0.04584709f;
    yuv[2] = r * -0.081014709086133f - g * 0.272538676238785f + b * 0.353553390593274f;
}

/* ConvertFromFakeBT709, ETC.cpp:2354-2364 */
static inline void etc_from_fake709(float rgb[3], const float yuv[3])
{
    float yy = yuv[0] * 0.57735026466774571071f;
    float u = yuv[1], v = yuv[2];
    rgb[0] = yy + u * 1.5748000207960953486f;
    rgb[1] = yy - u * 0.46812425854364753669f - v * 0.26491652528157560861f;
    rgb[2] = yy + v * 2.6242146882856944069f;
}

/* ComputeErrorFakeBT709, ETC.cpp:82-92 */
static inline float etc_error_fake(const int rec[3], const float pw[3])
{
    float yuv[3];
    etc_to_fake709(yuv, (float)rec[0], (float)rec[1], (float)rec[2]);
    float dy = yuv[0] - pw[0], du = yuv[1] - pw[1], dv = yuv[2] - pw[2];
    return dy * dy + du * du + dv * dv;
}

/* ResolveTHFakeBT709Rounding, ETC.cpp:2286-2327 (the error sums du + du, not du * du) */
static void etc_resolve_th_fake(int quantized[3], const int targets[3], int granularity)
{
    float lowF[3], highF[3];
    for (int ch = 0; ch < 3; ch++)
    {
        int unq = (quantized[ch] << 4) | quantized[ch];
        int next = unq + 17 < 255 ? unq + 17 : 255;
        lowF[ch] = (float)((int16_t)((int16_t)(unq * granularity) << 1));
        highF[ch] = (float)((int16_t)((int16_t)(next * granularity) << 1));
    }
    float bestError = FLT_MAX, cum[3];
    int bestOctant = 0;
    etc_to_fake709(cum, (float)targets[0], (float)targets[1], (float)targets[2]);
    for (int octant = 0; octant < 8; octant++)
    {
        float oy[3];
        etc_to_fake709(oy, (octant & 1) ? highF[0] : lowF[0], (octant & 2) ? highF[1] : lowF[1], (octant & 4) ? highF[2] : lowF[2]);
        float d0 = oy[0] - cum[0], d1 = oy[1] - cum[1], d2 = oy[2] - cum[2];
        float error = d0 * d0 + d1 + d1 + d2 * d2;
        if (error < bestError) bestOctant = octant;
        bestError = f_min(error, bestError);
    }
    for (int ch = 0; ch < 3; ch++)
        quantized[ch] = quantized[ch] + ((bestOctant >> ch) & 1);
}

/* ResolveHalfBlockFakeBT709RoundingAccurate / Fast, ETC.cpp:2157-2284 */
static void etc_resolve_half_fake(const etc_ctx_t *cx, int quantized[3], const int cumulative[3], int isDifferential)
{
    if (cx->fakeAccurate)
    {
        float lowF[3], highF[3];
        for (int ch = 0; ch < 3; ch++)
        {
            unsigned cu = (unsigned)cumulative[ch];
            if (isDifferential)
                quantized[ch] = (int)(((((cu << 5) - cu) + (cu >> 3)) & 0xffffu) >> 11);
            else
                quantized[ch] = (int)(((((cu << 5) - ((cu << 1) & 0xffffu)) + (cu >> 3)) & 0xffffu) >> 12);
            int unq, next;
            if (isDifferential)
            {
                unq = (quantized[ch] << 3) | (quantized[ch] >> 2);
                int qn = quantized[ch] + 1 < 31 ? quantized[ch] + 1 : 31;
                next = (qn << 3) | (qn >> 2);
            }
            else
            {
                unq = (quantized[ch] << 4) | quantized[ch];
                next = unq + 17 < 255 ? unq + 17 : 255;
            }
            lowF[ch] = (float)(unq << 3);
            highF[ch] = (float)(next << 3);
        }
        float bestError = FLT_MAX, cum[3];
        int bestOctant = 0;
        etc_to_fake709(cum, (float)cumulative[0], (float)cumulative[1], (float)cumulative[2]);
        for (int octant = 0; octant < 8; octant++)
        {
            float oy[3];
            etc_to_fake709(oy, (octant & 1) ? highF[0] : lowF[0], (octant & 2) ? highF[1] : lowF[1], (octant & 4) ? highF[2] : lowF[2]);
            float d0 = oy[0] - cum[0], d1 = oy[1] - cum[1], d2 = oy[2] - cum[2];
            float error = d0 * d0 + d1 + d1 + d2 * d2;
            if (error < bestError) bestOctant = octant;
            bestError = f_min(error, bestError);
        }
        for (int ch = 0; ch < 3; ch++)
            quantized[ch] = quantized[ch] + ((bestOctant >> ch) & 1);
        return;
    }
    int fill[3], base[3], rOff, gOff, bOff, upper;
    for (int ch = 0; ch < 3; ch++)
        fill[ch] = cumulative[ch] + (cumulative[ch] >> 8);
    if (isDifferential)
    {
        rOff = (fill[0] << 6) & 0xf00;
        gOff = (fill[1] << 4) & 0x0f0;
        bOff = (fill[2] >> 2) & 0x00f;
        for (int ch = 0; ch < 3; ch++)
            base[ch] = fill[ch] >> 6;
        upper = 31;
    }
    else
    {
        rOff = (fill[0] << 5) & 0xf00;
        gOff = (fill[1] << 1) & 0x0f0;
        bOff = (fill[2] >> 3) & 0x00f;
        for (int ch = 0; ch < 3; ch++)
            base[ch] = fill[ch] >> 7;
        upper = 15;
    }
    const int octant = orc_fake709_rounding16[rOff | gOff | bOff];
    for (int ch = 0; ch < 3; ch++)
    {
        int q = base[ch] + ((octant >> ch) & 1);
        quantized[ch] = q < upper ? q : upper;
    }
}

/* the metric most call sites use: fake BT.709 first, then uniform, then weighted (e.g. ETC.cpp:128-135) */
static inline float etc_error_wu(const etc_ctx_t *cx, const int rec[3], const int px[3], const float pw[3]);
static inline float etc_error(const etc_ctx_t *cx, const int rec[3], const int px[3], const float pw[3])
{
    if (cx->fake)
        return etc_error_fake(rec, pw);
    return etc_error_wu(cx, rec, px, pw);
}

/* ComputeErrorUniform / ComputeErrorWeighted, ETC.cpp:59-80.  The line colours of the T modes are measured with this
 * even under ETC_UseFakeBT709 (ETC.cpp:600, 1133, 1150), against pre-weighted pixels that then hold luma/chroma */
static inline float etc_error_wu(const etc_ctx_t *cx, const int rec[3], const int px[3], const float pw[3])
{
    if (cx->uniform)
    {
        float fd0 = (float)(rec[0] - px[0]);
        float error = fd0 * fd0;
        for (int ch = 1; ch < 3; ch++)
        {
            float fd = (float)(rec[ch] - px[ch]);
            error = error + fd * fd;
        }
        return error;
    }
    float dr = (float)rec[0] * cx->rw - pw[0];
    float dg = (float)rec[1] * cx->gw - pw[1];
    float db = (float)rec[2] * cx->bw - pw[2];
    return dr * dr + dg * dg + db * db;
}

static void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

static const int etc_selector_order[16] = {0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15};
static const int etc_flip_tables[2][2][8] = {
    {{0, 1, 4, 5, 8, 9, 12, 13}, {2, 3, 6, 7, 10, 11, 14, 15}},
    {{0, 1, 2, 3, 4, 5, 6, 7}, {8, 9, 10, 11, 12, 13, 14, 15}},
};

/* ---- planar, ETC.cpp:1266-1662 ---- */
static int planar_decode(int coeff, int ch)
{
    if (ch == 1)
        return ((coeff << 1) | (coeff >> 6)) & 0xffff;
    return ((coeff << 2) | (coeff >> 4)) & 0xffff;
}

static void etc2_planar(const etc_ctx_t *cx, etc_lane_t *ln)
{
    float h[3], v[3], o[3];
    float totalError = 0.0f;
    int bestCoeffs[3][3];
    memset(bestCoeffs, 0, sizeof(bestCoeffs));
    for (int ch = 0; ch < 3; ch++)
    {
        float fhh = 0.f, fho = 0.f, fhv = 0.f, foo = 0.f, fov = 0.f, fvv = 0.f;
        float fc = 0.0f, fh = 0.0f, fv = 0.0f, fo = 0.0f;
        for (int px = 0; px < 16; px++)
        {
            float x = (float)(px % 4);
            float y = (float)(px / 4);
            float c = cx->fake ? ln->pw[px][ch] : (float)ln->pixels[px][ch];
            fhh += x * x; fhv += x * y; fho += x; fh = fh - c * x;
            fhv += y * x; fvv += y * y; fov += y; fv = fv - c * y;   /* fvh, fvo alias fhv, fov */
            fho += x; fov += y; foo += 1; fo = fo - c;               /* foh aliases fho */
            fh = fh - c * x; fv = fv - c * y; fo = fo - c; fc = fc + c * c;
        }
        float d = 2.0f * fhh, e = fho, f = fhv, gD = fh;
        float i = fhv, j = fov, k = 2.0f * fvv, lD = fv;
        float m = fho, n = 2.0f * foo, p = fov, qD = fo;
        float r0to1 = -i / d, r0to2 = -m / d;
        float j1 = j + r0to1 * e, k1 = k + r0to1 * f, l1D = lD + gD * r0to1;
        float n1 = n + r0to2 * e, p1 = p + r0to2 * f, q1D = qD + gD * r0to2;
        float r1to2 = -p1 / k1;
        float n2 = n1 + r1to2 * j1, q2D = q1D + l1D * r1to2;
        o[ch] = -q2D / n2;
        float r2to1 = -j1 / n2;
        float l2D = l1D + q2D * r2to1;
        float elim2 = -f / k1, elim1 = -e / n2;
        float g2D = gD + l2D * elim2 + q2D * elim1;
        h[ch] = -g2D / d;
        v[ch] = -l2D / k1;
        h[ch] = h[ch] * 4.0f + o[ch];
        v[ch] = v[ch] * 4.0f + o[ch];
        (void)fc;
    }
    if (cx->fake)
    {
        /* ETC.cpp:1415-1474: back to RGB, round to nearest, one candidate, error in the fake space */
        float oRGB[3], hRGB[3], vRGB[3];
        etc_from_fake709(oRGB, o);
        etc_from_fake709(hRGB, h);
        etc_from_fake709(vRGB, v);
        int reconstructed[16][3];
        for (int ch = 0; ch < 3; ch++)
        {
            float fcoeffs[3] = {oRGB[ch], hRGB[ch], vRGB[ch]};
            for (int c = 0; c < 3; c++)
            {
                float coeff = f_max(0.0f, fcoeffs[c]);
                if (ch == 1)
                    coeff = f_min(127.0f, coeff * (127.0f / 255.0f));
                else
                    coeff = f_min(63.0f, coeff * (63.0f / 255.0f));
                bestCoeffs[ch][c] = coeff != coeff ? -32768 : (int)lrintf(coeff); /* cvtps2dq, round to nearest even */
            }
            int dO = planar_decode(bestCoeffs[ch][0], ch), dH = planar_decode(bestCoeffs[ch][1], ch), dV = planar_decode(bestCoeffs[ch][2], ch);
            int hMinusO = (int16_t)(dH - dO), vMinusO = (int16_t)(dV - dO);
            int addend = (int16_t)((dO << 2) + 2);
            for (int px = 0; px < 16; px++)
            {
                int x = px & 3, y = px >> 2;
                int interpolated = (int16_t)(x * hMinusO + y * vMinusO + addend) >> 2;
                int dec = interpolated < 0 ? 0 : interpolated;
                reconstructed[px][ch] = dec > 255 ? 255 : dec;
            }
        }
        for (int px = 0; px < 16; px++)
            totalError = totalError + etc_error_fake(reconstructed[px], ln->pw[px]);
    }
    else
    for (int ch = 0; ch < 3; ch++)
    {
        float fcoeffs[3] = {o[ch], h[ch], v[ch]};
        int ranges[3][2];
        for (int c = 0; c < 3; c++)
        {
            float coeff = f_max(0.0f, fcoeffs[c]);
            if (ch == 1)
                coeff = f_min(127.0f, coeff * (127.0f / 255.0f));
            else
                coeff = f_min(63.0f, coeff * (63.0f / 255.0f));
            /* RoundDownForScope / RoundUpForScope conversions, ETC.cpp:1495-1505 */
            int lo = (int)floorf(coeff), hi = (int)ceilf(coeff);
            if (coeff != coeff) lo = hi = -32768;
            ranges[c][0] = lo;
            ranges[c][1] = hi;
        }
        float bestChannelError = FLT_MAX;
        for (int io = 0; io < 2; io++)
        {
            int dO = planar_decode(ranges[0][io], ch);
            for (int ih = 0; ih < 2; ih++)
            {
                int dH = planar_decode(ranges[1][ih], ch);
                int hMinusO = (int16_t)(dH - dO);
                for (int iv = 0; iv < 2; iv++)
                {
                    int dV = planar_decode(ranges[2][iv], ch);
                    int vMinusO = (int16_t)(dV - dO);
                    float error = 0.0f;
                    int addend = (int16_t)((dO << 2) + 2);
                    for (int px = 0; px < 16; px++)
                    {
                        int x = px & 3, y = px >> 2;
                        int interpolated = (int16_t)(x * hMinusO + y * vMinusO + addend) >> 2;
                        int dec = interpolated < 0 ? 0 : interpolated;
                        if (dec > 255) dec = 255;
                        float deltaF = (float)(int16_t)(ln->pixels[px][ch] - dec);
                        error = error + deltaF * deltaF;
                    }
                    if (error < bestChannelError)
                    {
                        bestChannelError = f_min(error, bestChannelError);
                        bestCoeffs[ch][0] = ranges[0][io];
                        bestCoeffs[ch][1] = ranges[1][ih];
                        bestCoeffs[ch][2] = ranges[2][iv];
                    }
                }
            }
        }
        if (!cx->uniform)
        {
            float w = ch == 0 ? cx->rw : (ch == 1 ? cx->gw : cx->bw);
            bestChannelError = bestChannelError * (w * w);
        }
        totalError = totalError + bestChannelError;
    }
    if (totalError < ln->bestError)
    {
        ln->bestError = f_min(ln->bestError, totalError);
        int ro = bestCoeffs[0][0], rh = bestCoeffs[0][1], rv = bestCoeffs[0][2];
        int go = bestCoeffs[1][0], gh = bestCoeffs[1][1], gv = bestCoeffs[1][2];
        int bo = bestCoeffs[2][0], bh = bestCoeffs[2][1], bv = bestCoeffs[2][2];
        int go1 = go >> 6, go2 = go & 63;
        int bo1 = bo >> 5, bo2 = (bo >> 3) & 3, bo3 = bo & 7;
        int rh1 = rh >> 1, rh2 = rh & 1;
        int fakeR = ro >> 2, fakeDR = go1 | ((ro & 3) << 1);
        int fakeG = go2 >> 2, fakeDG = ((go2 & 3) << 1) | bo1;
        int fakeB = bo2, fakeDB = bo3 >> 1;
        uint32_t highBits = 0, lowBits = 0;
        if ((fakeDR & 4) != 0 && fakeR + fakeDR < 8) highBits |= 1u << (63 - 32);
        if ((fakeDG & 4) != 0 && fakeG + fakeDG < 8) highBits |= 1u << (55 - 32);
        if (fakeB + fakeDB < 4) highBits |= 1u << (42 - 32); else highBits |= 7u << (45 - 32);
        highBits |= (uint32_t)ro << (57 - 32);
        highBits |= (uint32_t)go1 << (56 - 32);
        highBits |= (uint32_t)go2 << (49 - 32);
        highBits |= (uint32_t)bo1 << (48 - 32);
        highBits |= (uint32_t)bo2 << (43 - 32);
        highBits |= (uint32_t)bo3 << (39 - 32);
        highBits |= (uint32_t)rh1 << (34 - 32);
        highBits |= 1u << (33 - 32);
        highBits |= (uint32_t)rh2 << (32 - 32);
        lowBits |= (uint32_t)gh << 25;
        lowBits |= (uint32_t)bh << 19;
        lowBits |= (uint32_t)rv << 13;
        lowBits |= (uint32_t)gv << 6;
        lowBits |= (uint32_t)bv << 0;
        put_be32(ln->out, highBits);
        put_be32(ln->out + 4, lowBits);
    }
}

/* ---- sector split along the chroma principal axis, ETC.cpp:1723-1848 ---- */
static void etc2_sector_assignments(const etc_ctx_t *cx, etc_lane_t *ln)
{
    float chromaDelta[16][2];
    if (cx->uniform)
    {
        int cc[16][2], cen[2] = {0, 0};
        for (int px = 0; px < 16; px++)
        {
            cc[px][0] = (int16_t)(ln->pixels[px][0] - ln->pixels[px][2]);
            cc[px][1] = (int16_t)(ln->pixels[px][0] - (ln->pixels[px][1] << 1) + ln->pixels[px][2]);
        }
        for (int px = 0; px < 16; px++)
            for (int ch = 0; ch < 2; ch++)
                cen[ch] = (int16_t)(cen[ch] + cc[px][ch]);
        for (int px = 0; px < 16; px++)
            for (int ch = 0; ch < 2; ch++)
                chromaDelta[px][ch] = cx->punchthrough ? (float)(int16_t)((int16_t)(cc[px][ch] * ln->numOpaque) - cen[ch])
                                                       : (float)(int16_t)((int16_t)(cc[px][ch] << 4) - cen[ch]);
        for (int px = 0; px < 16; px++)
            chromaDelta[px][1] = chromaDelta[px][1] * 0.57735026918962576450914878050196f;
    }
    else
    {
        float cc[16][2], cen[2] = {0.0f, 0.0f};
        for (int px = 0; px < 16; px++)
        {
            const float *p = ln->pw[px];
            cc[px][0] = p[0] * cx->axis0[0] + p[1] * cx->axis0[1] + p[2] * cx->axis0[2];
            cc[px][1] = p[0] * cx->axis1[0] + p[1] * cx->axis1[1] + p[2] * cx->axis1[2];
        }
        for (int px = 0; px < 16; px++)
            for (int ch = 0; ch < 2; ch++)
                cen[ch] = cen[ch] + cc[px][ch];
        for (int px = 0; px < 16; px++)
            for (int ch = 0; ch < 2; ch++)
                chromaDelta[px][ch] = cc[px][ch] * (cx->punchthrough ? (float)ln->numOpaque : 16.0f) - cen[ch];
    }
    float covXX = 0.0f, covYY = 0.0f, covXY = 0.0f;
    for (int px = 0; px < 16; px++)
    {
        float nx = chromaDelta[px][0], ny = chromaDelta[px][1];
        covXX = covXX + nx * nx;
        covYY = covYY + ny * ny;
        covXY = covXY + nx * ny;
    }
    float halfTrace = (covXX + covYY) * 0.5f;
    float det = covXX * covYY - covXY * covXY;
    float mm = sqrtf(f_max(0.0f, halfTrace * halfTrace - det));
    float ev = halfTrace + mm;
    float dx = (covYY - ev + covXY);
    float dy = -(covXX - ev + covXY);
    if (dx == 0.0f && dy == 0.0f)
        dx = 1.f;
    for (int px = 0; px < 16; px++)
        ln->isolated[px] = (chromaDelta[px][0] * dx + chromaDelta[px][1] * dy) < 0.0f;
}

/* ---- T mode, ETC.cpp:396-647 ---- */
typedef struct
{
    int isolatedQ[3];
    int lineTotal[3];
    int numLine;
    float isolatedError[16];
} tmode_setup_t;

static void tmode_setup(const etc_ctx_t *cx, const etc_lane_t *ln, const int *isIsolated, tmode_setup_t *ts)
{
    int isolatedTotal[3] = {0, 0, 0}, lineTotal[3] = {0, 0, 0}, numIsolated = 0;
    for (int px = 0; px < 16; px++)
    {
        for (int ch = 0; ch < 3; ch++)
        {
            if (isIsolated[px]) isolatedTotal[ch] += ln->pixels[px][ch];
            lineTotal[ch] += ln->pixels[px][ch];
        }
        numIsolated += isIsolated[px] ? 1 : 0;
    }
    for (int ch = 0; ch < 3; ch++)
        ts->lineTotal[ch] = lineTotal[ch] - isolatedTotal[ch];
    ts->numLine = 16 - numIsolated;
    const int divisor = numIsolated * 34;
    const int addend = (numIsolated << 4) | numIsolated;
    int isolatedColor[3], targets[3];
    for (int ch = 0; ch < 3; ch++)
    {
        int numerator = isolatedTotal[ch] + isolatedTotal[ch] + (cx->fake ? 0 : addend);
        ts->isolatedQ[ch] = divisor == 0 ? 0 : (numerator & 0xffff) / divisor;
        targets[ch] = numerator;
    }
    if (cx->fake)
        etc_resolve_th_fake(ts->isolatedQ, targets, numIsolated);
    for (int ch = 0; ch < 3; ch++)
        isolatedColor[ch] = ts->isolatedQ[ch] | (ts->isolatedQ[ch] << 4);
    for (int px = 0; px < 16; px++)
        ts->isolatedError[px] = etc_error(cx, isolatedColor, ln->pixels[px], ln->pw[px]);
}

/* unique line colours of one table for this lane (own premultiplier range; the reference's
 * group-wide range only adds clamped repeats that the consecutive de-duplication removes) */
static int tmode_unique(const etc_ctx_t *cx, const tmode_setup_t *ts, int table, int colors[34])
{
    const int modifier = orc_th_distance[table];
    const int modifierOffset = modifier + modifier;
    const int lineDivisor = ts->numLine * 34;
    const int lineAddend = (ts->numLine << 4) | ts->numLine;
    int n = 0;
    for (int k = -ts->numLine; k <= ts->numLine; k++)
    {
        int modifierAddend = (int16_t)(k * modifierOffset);
        int packed = 0, q[3], targets[3];
        for (int ch = 0; ch < 3; ch++)
        {
            int base = (int16_t)(ts->lineTotal[ch] + ts->lineTotal[ch] + (cx->fake ? 0 : lineAddend));
            int numerator = (int16_t)(base + modifierAddend);
            if (numerator < 0) numerator = 0;
            int divided = lineDivisor == 0 ? 0 : numerator / lineDivisor;
            q[ch] = divided < 15 ? divided : 15;
            targets[ch] = numerator;
        }
        if (cx->fake)
            etc_resolve_th_fake(q, targets, ts->numLine); /* ETC.cpp:511-531; never leaves 0 .. 15 over the swept domain (DESIGN.md 2.1) */
        for (int ch = 0; ch < 3; ch++)
            packed |= q[ch] << (ch * 5);
        if (n == 0 || packed != colors[n - 1])
            colors[n++] = packed;
    }
    return n;
}

static void etc2_emit_t(uint8_t *out, const int lineColor[3], const int isolatedColor[3], uint32_t packedSelectors, int table, int opaque)
{
    uint32_t lowBits = 0, highBits = 0;
    int rh = (isolatedColor[0] >> 2) & 3, rl = isolatedColor[0] & 3;
    if (rh + rl < 4) highBits |= 1u << (58 - 32); else highBits |= 7u << (61 - 32);
    highBits |= (uint32_t)rh << (59 - 32);
    highBits |= (uint32_t)rl << (56 - 32);
    highBits |= (uint32_t)isolatedColor[1] << (52 - 32);
    highBits |= (uint32_t)isolatedColor[2] << (48 - 32);
    highBits |= (uint32_t)lineColor[0] << (44 - 32);
    highBits |= (uint32_t)lineColor[1] << (40 - 32);
    highBits |= (uint32_t)lineColor[2] << (36 - 32);
    highBits |= (uint32_t)((table >> 1) & 3) << (34 - 32);
    if (opaque) highBits |= 1u << (33 - 32);
    highBits |= (uint32_t)(table & 1) << (32 - 32);
    for (int px = 0; px < 16; px++)
    {
        int sel = (packedSelectors >> (2 * etc_selector_order[px])) & 3;
        if (sel & 1) lowBits |= 1u << px;
        if (sel & 2) lowBits |= 1u << (16 + px);
    }
    put_be32(out, highBits);
    put_be32(out + 4, lowBits);
}

static void etc2_tmode(const etc_ctx_t *cx, etc_lane_t *ln, const int *isIsolated, const int groupMaxUnique[8])
{
    tmode_setup_t ts;
    tmode_setup(cx, ln, isIsolated, &ts);
    int bestIsThisMode = 0, bestTable = 0, bestLineColor = 0;
    uint32_t bestSelectors = 0;
    for (int table = 0; table < 8; table++)
    {
        int colors[40];
        memset(colors, 0, sizeof(colors)); /* canonical build: the array starts zeroed (hazard H2) */
        int n = tmode_unique(cx, &ts, table, colors);
        const int maxUnique = groupMaxUnique[table];
        for (int fill = n + 1; fill < maxUnique; fill++)
            colors[fill] = colors[0];
        const int modifier = orc_th_distance[table];
        for (int ci = 0; ci < maxUnique; ci++)
        {
            int lineColors[3][3];
            for (int ch = 0; ch < 3; ch++)
            {
                int q = (colors[ci] >> (ch * 5)) & 15;
                int u = (q << 4) | q;
                lineColors[0][ch] = u + modifier < 255 ? u + modifier : 255;
                lineColors[1][ch] = u;
                lineColors[2][ch] = u - modifier > 0 ? u - modifier : 0;
            }
            uint32_t selectors = 0;
            float error = 0.0f;
            for (int px = 0; px < 16; px++)
            {
                float pixelError = ts.isolatedError[px];
                int sel = 0;
                for (int i = 0; i < 3; i++)
                {
                    float e = etc_error_wu(cx, lineColors[i], ln->pixels[px], ln->pw[px]); /* sic: never the fake metric */
                    int better = e < pixelError;
                    pixelError = f_min(e, pixelError);
                    if (better) sel = i + 1;
                }
                error = error + pixelError;
                selectors |= (uint32_t)sel << (px * 2);
            }
            int better = error < ln->bestError;
            ln->bestError = f_min(error, ln->bestError);
            if (better)
            {
                bestLineColor = colors[ci];
                bestSelectors = selectors;
                bestTable = table;
                bestIsThisMode = 1;
            }
        }
    }
    if (bestIsThisMode)
    {
        int lineColor[3];
        for (int ch = 0; ch < 3; ch++)
            lineColor[ch] = (bestLineColor >> (ch * 5)) & 15;
        etc2_emit_t(ln->out, lineColor, ts.isolatedQ, bestSelectors, bestTable, 1);
    }
}

/* ---- H mode, ETC.cpp:649-885, EmitHModeBlock 2462-2563 ---- */
static void etc2_emit_h(uint8_t *out, const int blockColors[2], unsigned sectorBits, unsigned signBits, int table, int opaque)
{
    if (blockColors[0] == blockColors[1])
    {
        int lineColor[3], isolatedColor[3];
        lineColor[0] = isolatedColor[0] = (blockColors[0] >> 10) & 0x1f;
        lineColor[1] = isolatedColor[1] = (blockColors[0] >> 5) & 0x1f;
        lineColor[2] = isolatedColor[2] = (blockColors[0] >> 0) & 0x1f;
        uint32_t packedSelectors = 0x55555555u;
        for (int px = 0; px < 16; px++)
            packedSelectors |= (uint32_t)((signBits >> px) & 1) << ((px * 2) + 1);
        etc2_emit_t(out, lineColor, isolatedColor, packedSelectors, table, opaque);
        return;
    }
    int colors[2][3];
    for (int s = 0; s < 2; s++)
        for (int ch = 0; ch < 3; ch++)
            colors[s][ch] = (blockColors[s] >> ((2 - ch) * 5)) & 15;
    uint32_t lowBits = 0, highBits = 0;
    if (((table & 1) == 1) != (blockColors[0] > blockColors[1]))
    {
        for (int ch = 0; ch < 3; ch++)
        {
            int t = colors[0][ch]; colors[0][ch] = colors[1][ch]; colors[1][ch] = t;
        }
        sectorBits ^= 0xffff;
    }
    int r1 = colors[0][0], g1a = colors[0][1] >> 1, g1b = colors[0][1] & 1, b1a = colors[0][2] >> 3, b1b = colors[0][2] & 7;
    int r2 = colors[1][0], g2 = colors[1][1], b2 = colors[1][2];
    if ((g1a & 4) != 0 && r1 + g1a < 8) highBits |= 1u << (63 - 32);
    int fakeDG = b1b >> 1, fakeG = b1a | (g1b << 1);
    if (fakeG + fakeDG < 4) highBits |= 1u << (50 - 32); else highBits |= 7u << (53 - 32);
    int da = (table >> 2) & 1, db = (table >> 1) & 1;
    highBits |= (uint32_t)r1 << (59 - 32);
    highBits |= (uint32_t)g1a << (56 - 32);
    highBits |= (uint32_t)g1b << (52 - 32);
    highBits |= (uint32_t)b1a << (51 - 32);
    highBits |= (uint32_t)b1b << (47 - 32);
    highBits |= (uint32_t)r2 << (43 - 32);
    highBits |= (uint32_t)g2 << (39 - 32);
    highBits |= (uint32_t)b2 << (35 - 32);
    highBits |= (uint32_t)da << (34 - 32);
    if (opaque) highBits |= 1u << (33 - 32);
    highBits |= (uint32_t)db << (32 - 32);
    for (int px = 0; px < 16; px++)
    {
        int sectorBit = (sectorBits >> etc_selector_order[px]) & 1;
        int signBit = (signBits >> etc_selector_order[px]) & 1;
        lowBits |= (uint32_t)signBit << px;
        lowBits |= (uint32_t)sectorBit << (16 + px);
    }
    put_be32(out, highBits);
    put_be32(out + 4, lowBits);
}

static void etc2_hmode(const etc_ctx_t *cx, etc_lane_t *ln, const int *groupings)
{
    int counts[2] = {0, 0}, totals[2][3] = {{0, 0, 0}, {0, 0, 0}};
    for (int px = 0; px < 16; px++)
    {
        for (int ch = 0; ch < 3; ch++)
        {
            totals[0][ch] += ln->pixels[px][ch];
            if (groupings[px]) totals[1][ch] += ln->pixels[px][ch];
        }
        counts[1] += groupings[px] ? 1 : 0;
    }
    for (int ch = 0; ch < 3; ch++)
        totals[0][ch] -= totals[1][ch];
    counts[0] = 16 - counts[1];

    unsigned bestSectorBits = 0, bestSignBits = 0;
    int bestColors[2] = {0, 0}, bestTable = 0, bestIsThisMode = 0;
    for (int table = 0; table < 8; table++)
    {
        const int modifier = orc_th_distance[table];
        int unique[70], numUnique[2];
        int total = 0;
        for (int sector = 0; sector < 2; sector++)
        {
            int n = 0;
            const int cnt = counts[sector];
            for (int k = -cnt; k <= cnt; k++)
            {
                int q[3];
                for (int ch = 0; ch < 3; ch++)
                {
                    if (cnt == 0)
                        q[ch] = 0;
                    else
                    {
                        int v = (int16_t)(totals[sector][ch] * 2 + cnt * 17 + modifier * 2 * k);
                        if (v < 0) v = 0;
                        v = v / (cnt * 34);
                        q[ch] = v < 15 ? v : 15;
                    }
                }
                int packed = (q[0] << 10) | (q[1] << 5) | q[2];
                if (n == 0 || packed != unique[total + n - 1])
                    unique[total + n++] = packed;
            }
            numUnique[sector] = n;
            total += n;
        }
        static __thread float errors[70][16];
        unsigned signs[70];
        for (int ci = 0; ci < total; ci++)
        {
            int colors[2][3];
            for (int ch = 0; ch < 3; ch++)
            {
                int q = (unique[ci] >> ((2 - ch) * 5)) & 15;
                int u = (q << 4) | q;
                colors[0][ch] = u + modifier < 255 ? u + modifier : 255;
                colors[1][ch] = u - modifier > 0 ? u - modifier : 0;
            }
            unsigned signBits = 0;
            for (int px = 0; px < 16; px++)
            {
                float e0 = etc_error(cx, colors[0], ln->pixels[px], ln->pw[px]);
                float e1 = etc_error(cx, colors[1], ln->pixels[px], ln->pw[px]);
                if (e1 < e0) signBits |= 1u << px;
                errors[ci][px] = f_min(e0, e1);
            }
            signs[ci] = signBits;
        }
        /* colour pairs in the reference's odometer order (ETC.cpp:797-812): (1,0),(2,0),...,
         * the pair (0,0) is only reached when both lists have one entry */
        int idx0 = 0, idx1 = 0;
        const int combos = numUnique[0] * numUnique[1];
        for (int combo = 0; combo < combos; combo++)
        {
            int n0 = idx0 + 1, overflow = 0;
            if (n0 > numUnique[0] - 1)
            {
                n0 = 0;
                overflow = 1;
            }
            int n1 = idx1 + overflow;
            if (n1 > numUnique[1] - 1) n1 = numUnique[1] - 1;
            idx0 = n0;
            idx1 = n1;
            const int ci0 = idx0, ci1 = idx1 + numUnique[0];
            float totalError = 0.0f;
            unsigned sectorBits = 0, signBits = 0;
            for (int px = 0; px < 16; px++)
            {
                float e0 = errors[ci0][px], e1 = errors[ci1][px];
                totalError = totalError + f_min(e0, e1);
                int error1Better = e1 < e0;
                if (error1Better) sectorBits |= 1u << px;
                signBits |= (1u << px) & (error1Better ? signs[ci1] : signs[ci0]);
            }
            if (totalError < ln->bestError)
            {
                bestIsThisMode = 1;
                bestTable = table;
                bestColors[0] = unique[ci0];
                bestColors[1] = unique[ci1];
                bestSectorBits = sectorBits;
                bestSignBits = signBits;
                ln->bestError = f_min(totalError, ln->bestError);
            }
        }
    }
    if (bestIsThisMode)
        etc2_emit_h(ln->out, bestColors, bestSectorBits, bestSignBits, bestTable, 1);
}

/* ---- ETC1 differential cluster fit, ETC.cpp:2624-2882, 94-149, 219-362, 2565-2622 ---- */
typedef struct
{
    float error;
    uint16_t selectors, color;
    uint8_t table;
} etc_attempt_t;

static int etc_diff_legal(unsigned a, unsigned b)
{
    for (int sh = 10; sh >= 0; sh -= 5)
    {
        int d = (int)((b >> sh) & 31) - (int)((a >> sh) & 31);
        if (sh == 10) d = (int)(b >> 10) - (int)(a >> 10);
        if (!(-4 <= d && d <= 3)) return 0;
    }
    return 1;
}

/* minD = 1: the differential-only call CompressETC2Block makes (it passes punchthrough = true, ETC.cpp:1862);
 * minD = 0: CompressETC1Block (ETC.cpp:2116-2126), which also tries the individual 4:4:4 + 4:4:4 mode per flip */
static void etc1_cluster_fit(const etc_ctx_t *cx, etc_lane_t *ln, int minD)
{
    static __thread etc_attempt_t attempts[2][640];
    static __thread uint16_t sortIdx[2][640];
    int bestIsThisMode = 0, bestFlip = 0, bestD = 0;
    unsigned bestColors[2] = {0, 0}, bestSelectors[2] = {0, 0};
    int bestTables[2] = {0, 0};

    for (int flip = 0; flip < 2; flip++)
    for (int d = minD; d < 2; d++)
    {
        int numAttempts[2] = {0, 0};
        for (int sector = 0; sector < 2; sector++)
        {
            int cumulative[3] = {0, 0, 0};
            int spix[8][3];
            float spw[8][3];
            for (int px = 0; px < 8; px++)
                for (int ch = 0; ch < 3; ch++)
                {
                    int src = etc_flip_tables[flip][sector][px];
                    spix[px][ch] = ln->pixels[src][ch];
                    spw[px][ch] = ln->pw[src][ch];
                    cumulative[ch] += spix[px][ch];
                }
            for (int table = 0; table < 8; table++)
            {
                const int numOffsets = orc_cluster_count[table];
                const int16_t *offsets = orc_cluster_offsets + orc_cluster_start[table];
                unsigned colors[81];
                int n = 0;
                for (int oi = 0; oi < numOffsets; oi++)
                {
                    unsigned packed = 0;
                    if (cx->fake)
                    {
                        int offsetCumulative[3], q3[3];
                        for (int ch = 0; ch < 3; ch++)
                        {
                            int cu = (int16_t)(cumulative[ch] + offsets[oi]);
                            if (cu < 0) cu = 0;
                            if (cu > 2040) cu = 2040;
                            offsetCumulative[ch] = cu;
                        }
                        etc_resolve_half_fake(cx, q3, offsetCumulative, d == 1);
                        packed = (unsigned)q3[0] | ((unsigned)q3[1] << 5) | ((unsigned)q3[2] << 10);
                    }
                    else
                    for (int ch = 0; ch < 3; ch++)
                    {
                        int cu = (int16_t)(cumulative[ch] + offsets[oi]);
                        if (cu < 0) cu = 0;
                        if (cu > 2040) cu = 2040;
                        unsigned q = d == 1 ? ((((unsigned)cu << 5) - (unsigned)cu + ((unsigned)cu >> 3) + 1024u) & 0xffffu) >> 11
                                            : ((((unsigned)cu << 5) - ((unsigned)cu << 1) + ((unsigned)cu >> 3) + 2048u) & 0xffffu) >> 12;
                        packed |= q << (ch * 5);
                    }
                    if (n == 0 || packed != colors[n - 1])
                        colors[n++] = packed;
                }
                const int16_t *mods = orc_etc1_modifiers + table * 4;
                for (int i = 0; i < n; i++)
                {
                    /* TestHalfBlock */
                    int modified[4][3];
                    for (int ch = 0; ch < 3; ch++)
                    {
                        int q = (colors[i] >> (ch * 5)) & 31;
                        int u = d == 1 ? ((q << 3) | (q >> 2)) : ((q << 4) | q);
                        for (int s = 0; s < 4; s++)
                        {
                            int v = u + mods[s];
                            if (v < 0) v = 0;
                            if (v > 255) v = 255;
                            modified[s][ch] = v;
                        }
                    }
                    unsigned selectors = 0;
                    float totalError = 0.0f;
                    for (int px = 0; px < 8; px++)
                    {
                        float bestError = FLT_MAX;
                        unsigned bestSelector = 0;
                        for (unsigned s = 0; s < 4; s++)
                        {
                            float e = etc_error(cx, modified[s], spix[px], spw[px]);
                            if (e < bestError) bestSelector = s;
                            bestError = f_min(e, bestError);
                        }
                        totalError = totalError + bestError;
                        selectors |= bestSelector << (px * 2);
                    }
                    etc_attempt_t *a = &attempts[sector][numAttempts[sector]++];
                    a->error = totalError;
                    a->selectors = (uint16_t)selectors;
                    a->color = (uint16_t)colors[i];
                    a->table = (uint8_t)table;
                }
            }
        }

        if (d == 0)
        {
            /* individual mode: the cheapest attempt of each half, no constraint between them (ETC.cpp:2796-2851) */
            float bestInd[2] = {FLT_MAX, FLT_MAX};
            int which[2] = {0, 0};
            for (int sector = 0; sector < 2; sector++)
                for (int i = 0; i < numAttempts[sector]; i++)
                    if (attempts[sector][i].error < bestInd[sector])
                    {
                        bestInd[sector] = attempts[sector][i].error;
                        which[sector] = i;
                    }
            if (bestInd[0] + bestInd[1] < ln->bestError)
            {
                bestIsThisMode = 1;
                ln->bestError = bestInd[0] + bestInd[1];
                bestFlip = flip;
                bestD = 0;
                for (int sector = 0; sector < 2; sector++)
                {
                    bestColors[sector] = attempts[sector][which[sector]].color;
                    bestSelectors[sector] = attempts[sector][which[sector]].selectors;
                    bestTables[sector] = attempts[sector][which[sector]].table;
                }
            }
            continue;
        }

        /* FindBestDifferentialCombination(flip, d = 1, canIgnore = false) */
        float blockBest = ln->bestError;
        float bestDiffErrors[2] = {FLT_MAX, FLT_MAX};
        int bestAttempt[2] = {0, 0};
        for (int sector = 0; sector < 2; sector++)
            for (int i = 0; i < numAttempts[sector]; i++)
                if (attempts[sector][i].error < bestDiffErrors[sector])
                {
                    bestDiffErrors[sector] = attempts[sector][i].error;
                    bestAttempt[sector] = i;
                }
        if (bestDiffErrors[0] + bestDiffErrors[1] < blockBest)
        {
            const etc_attempt_t *a0 = &attempts[0][bestAttempt[0]], *a1 = &attempts[1][bestAttempt[1]];
            if (etc_diff_legal(a0->color, a1->color))
            {
                bestIsThisMode = 1;
                ln->bestError = bestDiffErrors[0] + bestDiffErrors[1];
                bestFlip = flip;
                bestD = 1;
                bestColors[0] = a0->color; bestColors[1] = a1->color;
                bestSelectors[0] = a0->selectors; bestSelectors[1] = a1->selectors;
                bestTables[0] = a0->table; bestTables[1] = a1->table;
            }
            else
            {
                int numSort[2] = {0, 0};
                for (int sector = 0; sector < 2; sector++)
                {
                    for (int i = 0; i < numAttempts[sector]; i++)
                        if (attempts[sector][i].error < blockBest)
                            sortIdx[sector][numSort[sector]++] = (uint16_t)i;
                    /* std::sort by (error, index): any correct sort gives the same order */
                    for (int i = 1; i < numSort[sector]; i++)
                    {
                        uint16_t key = sortIdx[sector][i];
                        float ke = attempts[sector][key].error;
                        int j = i - 1;
                        while (j >= 0)
                        {
                            uint16_t o = sortIdx[sector][j];
                            float oe = attempts[sector][o].error;
                            if (oe < ke || (!(oe > ke) && o < key))
                                break;
                            sortIdx[sector][j + 1] = o;
                            j--;
                        }
                        sortIdx[sector][j + 1] = key;
                    }
                }
                for (int i = 0; i < numSort[0]; i++)
                {
                    const etc_attempt_t *a0s = &attempts[0][sortIdx[0][i]];
                    float error0 = a0s->error;
                    if (error0 >= blockBest)
                        break;
                    float maxError1 = ln->bestError - error0;
                    if (maxError1 < bestDiffErrors[1])
                        break;
                    for (int j = 0; j < numSort[1]; j++)
                    {
                        const etc_attempt_t *a1s = &attempts[1][sortIdx[1][j]];
                        float error1 = a1s->error;
                        if (error1 >= maxError1)
                            break;
                        if (etc_diff_legal(a0s->color, a1s->color))
                        {
                            blockBest = error0 + error1;
                            bestIsThisMode = 1;
                            ln->bestError = blockBest;
                            bestFlip = flip;
                            bestD = 1;
                            bestColors[0] = a0s->color; bestColors[1] = a1s->color;
                            bestSelectors[0] = a0s->selectors; bestSelectors[1] = a1s->selectors;
                            bestTables[0] = a0s->table; bestTables[1] = a1s->table;
                            break;
                        }
                    }
                }
            }
        }
    }

    if (bestIsThisMode)
    {
        /* EmitETC1Block, ETC.cpp:2565-2622 */
        int colors[2][3];
        for (int s = 0; s < 2; s++)
            for (int ch = 0; ch < 3; ch++)
                colors[s][ch] = (bestColors[s] >> (ch * 5)) & 31;
        uint32_t highBits = 0, lowBits = 0;
        if (bestD == 0)
        {
            for (int ch = 0; ch < 3; ch++)
            {
                highBits |= (uint32_t)colors[0][ch] << (28 - 8 * ch);
                highBits |= (uint32_t)colors[1][ch] << (24 - 8 * ch);
            }
        }
        else
        {
            highBits |= (uint32_t)colors[0][0] << 27;
            highBits |= (uint32_t)((colors[1][0] - colors[0][0]) & 7) << 24;
            highBits |= (uint32_t)colors[0][1] << 19;
            highBits |= (uint32_t)((colors[1][1] - colors[0][1]) & 7) << 16;
            highBits |= (uint32_t)colors[0][2] << 11;
            highBits |= (uint32_t)((colors[1][2] - colors[0][2]) & 7) << 8;
        }
        highBits |= (uint32_t)bestTables[0] << 5;
        highBits |= (uint32_t)bestTables[1] << 2;
        highBits |= (uint32_t)bestD << 1;
        highBits |= (uint32_t)bestFlip;
        static const uint8_t modifierCodes[4] = {3, 2, 0, 1};
        uint8_t codes[16];
        for (int sector = 0; sector < 2; sector++)
            for (int px = 0; px < 8; px++)
                codes[etc_flip_tables[bestFlip][sector][px]] = modifierCodes[(bestSelectors[sector] >> (2 * px)) & 3];
        for (int sb = 0; sb < 2; sb++)
            for (int px = 0; px < 16; px++)
                lowBits |= (uint32_t)((codes[etc_selector_order[px]] >> sb) & 1) << (px + sb * 16);
        put_be32(ln->out, highBits);
        put_be32(ln->out + 4, lowBits);
    }
}

/* ---- EAC: 8-bit alpha and 11-bit R11 (CompressETC2AlphaBlockInternal, ETC.cpp:1902-2085; QuantizeETC2Alpha,
 * 2366-2411).  Integer only and lane independent; 16-bit lanes wrap like the reference's. ---- */
/* errOut: NULL, or where the final bestTotalError (the score of the emitted table, base, multiplier and indexes) goes */
static void eac_block(const int pixels[16], int is11Bit, int isSigned, uint8_t *out, uint32_t *errOut)
{
    int minAlpha = is11Bit ? 2047 : 255, maxAlpha = 0;
    for (int px = 0; px < 16; px++)
    {
        if (pixels[px] < minAlpha) minAlpha = pixels[px];
        if (pixels[px] > maxAlpha) maxAlpha = pixels[px];
    }
    const int alphaSpan = (uint16_t)(maxAlpha - minAlpha);
    const int alphaSpanMidpointTimes2 = maxAlpha + minAlpha;
    uint32_t bestTotalError = 0x7fffffffu;
    int bestTableIndex = 0, bestBaseCodeword = 0, bestMultiplier = 0;
    int bestIndexes[16];
    memset(bestIndexes, 0, sizeof(bestIndexes));

    for (int tableIndex = 0; tableIndex < 16; tableIndex++)
    {
        const uint8_t *pos = orc_eac_positive + tableIndex * 4;
        for (int r = 0; r < 10; r++)
        {
            int subrange = r % 3, mainRange = r / 3;
            int maxOffset = pos[3 - mainRange - (subrange & 1)];
            int minOffset = -(int)pos[3 - mainRange - ((subrange >> 1) & 1)] - 1;
            int offsetSpan = (uint16_t)(maxOffset - minOffset);
            int minMultiplier = alphaSpan / offsetSpan;
            if (is11Bit)
            {
                /* valid multipliers under 15, rounded down to a multiple of 8 */
                if (minMultiplier > 112) minMultiplier = 112;
                minMultiplier &= 120;
            }
            else
            {
                if (minMultiplier > 14) minMultiplier = 14;
                if (minMultiplier < 1) minMultiplier = 1;
            }
            for (int multiplierOffset = 0; multiplierOffset < 2; multiplierOffset++)
            {
                int multiplier = minMultiplier;
                if (is11Bit)
                {
                    if (multiplierOffset == 1) multiplier += 8;
                    else if (multiplier < 1) multiplier = 1;
                }
                else if (multiplierOffset == 1)
                    multiplier += 1;
                int multipliedMinOffset = (int16_t)(multiplier * minOffset);
                int multipliedMaxOffset = (int16_t)(multiplier * maxOffset);
                int unclampedBaseAlphaTimes2 = (int16_t)(alphaSpanMidpointTimes2 - multipliedMaxOffset - multipliedMinOffset);
                int baseAlpha;
                if (is11Bit)
                {
                    if (isSigned)
                        unclampedBaseAlphaTimes2 = (int16_t)(unclampedBaseAlphaTimes2 + 8);
                    const int minBase2 = isSigned ? 16 : 0;
                    int clamped = unclampedBaseAlphaTimes2 < minBase2 ? minBase2 : unclampedBaseAlphaTimes2;
                    if (clamped > 4095) clamped = 4095;
                    baseAlpha = (clamped >> 1) & 2040;
                    if (!isSigned)
                        baseAlpha += 4;
                }
                else
                {
                    int clamped = unclampedBaseAlphaTimes2 < 0 ? 0 : unclampedBaseAlphaTimes2;
                    if (clamped > 510) clamped = 510;
                    baseAlpha = (clamped + 1) >> 1;
                }

                int indexes[16];
                uint32_t totalError = 0;
                for (int px = 0; px < 16; px++)
                {
                    /* QuantizeETC2Alpha */
                    int offset = (int16_t)(pixels[px] - baseAlpha);
                    int offsetAboutReflectorTimes2 = (int16_t)(offset + offset + multiplier);
                    int absv = offsetAboutReflectorTimes2 < 0 ? -offsetAboutReflectorTimes2 : offsetAboutReflectorTimes2;
                    int lookupIndex = (absv & 0xffff) >> 1;
                    int blockLookupIndex = lookupIndex / multiplier;
                    if (blockLookupIndex >= 13) blockLookupIndex = 12;
                    int index = orc_eac_rounding[tableIndex * 13 + blockLookupIndex];
                    int positiveOffsetUnmultiplied = pos[index];
                    int signBits = offsetAboutReflectorTimes2 < 0 ? -1 : 0;
                    int offsetUnmultiplied = (int16_t)(positiveOffsetUnmultiplied ^ signBits);
                    int quantizedOffset = (int16_t)(offsetUnmultiplied * multiplier);
                    int offsetValue = (int16_t)(baseAlpha + quantizedOffset);
                    const int lo = (is11Bit && isSigned) ? 1 : 0, hi = is11Bit ? 2047 : 255;
                    int q = offsetValue < lo ? lo : offsetValue;
                    if (q > hi) q = hi;
                    indexes[px] = index + 4 - (signBits & 4);
                    if (is11Bit)
                    {
                        int delta = (int16_t)(q - pixels[px]);
                        totalError += (uint32_t)(delta * delta);
                    }
                    else
                    {
                        uint16_t d = (uint16_t)(q - pixels[px]);
                        totalError += (uint16_t)(d * d);
                    }
                }
                if (totalError < bestTotalError)
                {
                    bestTotalError = totalError;
                    bestTableIndex = tableIndex;
                    bestBaseCodeword = baseAlpha;
                    bestMultiplier = multiplier;
                    memcpy(bestIndexes, indexes, sizeof(indexes));
                }
            }
        }
    }
    if (errOut)
        *errOut = bestTotalError;
    if (is11Bit)
    {
        bestMultiplier >>= 3;
        if (isSigned)
            bestBaseCodeword ^= 0x80;
    }
    out[0] = (uint8_t)bestBaseCodeword;
    out[1] = (uint8_t)((bestMultiplier << 4) | bestTableIndex);
    int ordered[16];
    for (int px = 0; px < 16; px++)
        ordered[etc_selector_order[px]] = bestIndexes[px];
    int outputOffset = 2, outputBits = 0, numOutputBits = 0;
    for (int s = 0; s < 16; s++)
    {
        outputBits = (outputBits << 3) | ordered[s];
        numOutputBits += 3;
        if (numOutputBits >= 8)
        {
            out[outputOffset++] = (uint8_t)(outputBits >> (numOutputBits - 8));
            numOutputBits -= 8;
            outputBits &= ((1 << numOutputBits) - 1);
        }
    }
}

static void etc2_alpha_block(const uint8_t *block, uint8_t *out, uint32_t *errOut)
{
    int pixels[16];
    for (int px = 0; px < 16; px++)
        pixels[px] = block[px * 4 + 3];
    eac_block(pixels, 0, 0, out, errOut);
}

/* CompressEACBlock, ETC.cpp:2087-2114: PixelBlockScalarS16 -> shifted 11-bit range -> 8 bytes */
int orc_encode_eac11(uint8_t *out, const int16_t *blocksS16, size_t numBlocks, int isSigned)
{
    if (numBlocks % 8 != 0)
        return -1;
    for (size_t b = 0; b < numBlocks; b++)
    {
        int pixels[16];
        for (int px = 0; px < 16; px++)
        {
            int v = blocksS16[b * 16 + px];
            if (isSigned)
            {
                v = (int16_t)((v > 1023 ? 1023 : v) + 1024);
                if (v < 1) v = 1;
            }
            else
            {
                if (v > 2047) v = 2047;
                if (v < 0) v = 0;
            }
            pixels[px] = v;
        }
        eac_block(pixels, 1, isSigned, out + b * 8, NULL);
    }
    return 0;
}

/* ---- punch-through: EncodeVirtualTModePunchthrough, ETC.cpp:887-1264 ----
 * T and H mode with the third paint colour replaced by "transparent".  Colours here are packed r << 10 | g << 5 | b. */
typedef struct
{
    int isoQ[3];          /* isolatedAverageQuantized */
    int hIsoQ[8][3];      /* hModeIsolatedQuantized per table */
    float isolatedError[16];
    int lineTotal[3], numLine;
} vt_setup_t;

static void vt_setup(const etc_ctx_t *cx, const etc_lane_t *ln, const int *isIsolatedBase, vt_setup_t *vs)
{
    int isolatedTotal[3] = {0, 0, 0}, numIsolated = 0, isoTargets[3];
    vs->numLine = 0;
    for (int ch = 0; ch < 3; ch++)
        vs->lineTotal[ch] = 0;
    for (int px = 0; px < 16; px++)
    {
        const int opaque = !ln->transparent[px];
        const int iso = isIsolatedBase[px] && opaque, line = !isIsolatedBase[px] && opaque;
        for (int ch = 0; ch < 3; ch++)
        {
            if (iso) isolatedTotal[ch] += ln->pixels[px][ch];
            if (line) vs->lineTotal[ch] += ln->pixels[px][ch];
        }
        numIsolated += iso;
        vs->numLine += line;
    }
    const int divisor = numIsolated * 34;
    const int addend = (numIsolated << 4) | numIsolated;
    for (int ch = 0; ch < 3; ch++)
    {
        const int numerator = isolatedTotal[ch] + isolatedTotal[ch] + (cx->fake ? 0 : addend);
        vs->isoQ[ch] = divisor == 0 ? 0 : numerator / divisor;
        isoTargets[ch] = numerator;
        for (int table = 0; table < 8; table++)
        {
            const int offsetTotal = isolatedTotal[ch] + orc_th_distance[table] * numIsolated;
            int q = divisor == 0 ? 0 : (offsetTotal + offsetTotal + addend) / divisor;
            vs->hIsoQ[table][ch] = q < 15 ? q : 15;
        }
    }
    if (cx->fake)
        etc_resolve_th_fake(vs->isoQ, isoTargets, numIsolated);
    int isolatedColor[3];
    for (int ch = 0; ch < 3; ch++)
        isolatedColor[ch] = vs->isoQ[ch] | (vs->isoQ[ch] << 4);
    for (int px = 0; px < 16; px++)
        vs->isolatedError[px] = ln->transparent[px] ? 0.0f : etc_error(cx, isolatedColor, ln->pixels[px], ln->pw[px]);
}

/* unique line colours of one table: the premultiplier walks the GROUP's range in steps of two and is clamped to the
 * lane's own range (ETC.cpp:1025-1098), so the candidates depend on the group maximum of the line-pixel counts */
static int vt_unique(const etc_ctx_t *cx, const vt_setup_t *vs, int table, int clusterMaxLine, int colors[40])
{
    const int modifierOffset = orc_th_distance[table] * 2;
    const int lineDivisor = vs->numLine * 34;
    const int lineAddend = (vs->numLine << 4) | vs->numLine;
    int n = 0;
    for (int k = -clusterMaxLine; k <= clusterMaxLine; k += 2)
    {
        int kc = k < vs->numLine ? k : vs->numLine;
        kc = kc > -vs->numLine ? kc : -vs->numLine;
        const int modifierAddend = (int16_t)(kc * modifierOffset);
        int q[3], targets[3];
        for (int ch = 0; ch < 3; ch++)
        {
            int numerator = (int16_t)((int16_t)(vs->lineTotal[ch] + vs->lineTotal[ch] + (cx->fake ? 0 : lineAddend)) + modifierAddend);
            if (numerator < 0) numerator = 0;
            const int divided = lineDivisor == 0 ? 0 : numerator / lineDivisor;
            q[ch] = divided < 15 ? divided : 15;
            targets[ch] = numerator;
        }
        if (cx->fake)
            etc_resolve_th_fake(q, targets, vs->numLine);
        const int packed = (q[0] << 10) | (q[1] << 5) | q[2];
        if (n == 0 || packed != colors[n - 1])
            colors[n++] = packed;
    }
    return n;
}

static void etc2_virtual_tmode(const etc_ctx_t *cx, etc_lane_t *ln, const vt_setup_t *vs, int clusterMaxLine, const int groupMaxUnique[8])
{
    int bestIsThisMode = 0, bestIsH = 0, bestTable = 0, bestLineColor = 0, bestHColor2 = 0;
    uint32_t bestSelectors = 0;
    for (int table = 0; table < 8; table++)
    {
        int colors[40];
        memset(colors, 0, sizeof(colors)); /* canonical build: zeroed (hazard H2, same as the opaque T mode) */
        const int n = vt_unique(cx, vs, table, clusterMaxLine, colors);
        const int maxUnique = groupMaxUnique[table];
        for (int fill = n + 1; fill < maxUnique; fill++)
            colors[fill] = colors[0];
        const int modifier = orc_th_distance[table];
        int hColor[3];
        float hErrors[16];
        for (int ch = 0; ch < 3; ch++)
        {
            const int q = vs->hIsoQ[table][ch];
            const int u = (q << 4) | q;
            hColor[ch] = u - modifier > 0 ? u - modifier : 0;
        }
        for (int px = 0; px < 16; px++)
            hErrors[px] = ln->transparent[px] ? 0.0f : etc_error_wu(cx, hColor, ln->pixels[px], ln->pw[px]);
        const int packedH2 = (vs->hIsoQ[table][0] << 10) | (vs->hIsoQ[table][1] << 5) | vs->hIsoQ[table][2];
        const int tableLowBitIsZero = (table & 1) == 0;
        for (int ci = 0; ci < maxUnique; ci++)
        {
            int lineColors[2][3];
            for (int ch = 0; ch < 3; ch++)
            {
                const int q = (colors[ci] >> (10 - ch * 5)) & 15;
                const int u = (q << 4) | q;
                lineColors[0][ch] = u + modifier < 255 ? u + modifier : 255;
                lineColors[1][ch] = u - modifier > 0 ? u - modifier : 0;
            }
            int lineSel[16];
            float lineErr[16], tErr = 0.0f, hErr = 0.0f;
            for (int px = 0; px < 16; px++)
            {
                const float e0 = etc_error_wu(cx, lineColors[0], ln->pixels[px], ln->pw[px]);
                const float e1 = etc_error_wu(cx, lineColors[1], ln->pixels[px], ln->pw[px]);
                lineSel[px] = e0 <= e1 ? 1 : 3;
                lineErr[px] = ln->transparent[px] ? 0.0f : f_min(e0, e1);
            }
            for (int px = 0; px < 16; px++)
            {
                tErr = tErr + f_min(lineErr[px], vs->isolatedError[px]);
                hErr = hErr + f_min(lineErr[px], hErrors[px]);
            }
            const int hLegal = (colors[ci] < packedH2) == tableLowBitIsZero;
            const int useH = (hErr < tErr) && hLegal;
            const float roundBest = useH ? hErr : tErr;
            if (roundBest < ln->bestError)
            {
                uint32_t selectors = 0;
                for (int px = 0; px < 16; px++)
                {
                    int sel = lineSel[px];
                    if ((useH ? hErrors[px] : vs->isolatedError[px]) < lineErr[px]) sel = 0;
                    if (ln->transparent[px]) sel = 2;
                    selectors |= (uint32_t)sel << (px * 2);
                }
                ln->bestError = roundBest;
                bestLineColor = colors[ci];
                bestSelectors = selectors;
                bestTable = table;
                bestIsH = useH;
                bestHColor2 = packedH2;
                bestIsThisMode = 1;
            }
        }
    }
    if (!bestIsThisMode)
        return;
    if (bestIsH)
    {
        static const unsigned remapSector[4] = {1, 0, 1, 0}, remapSign[4] = {1, 0, 0, 1};
        unsigned signBits = 0, sectorBits = 0;
        for (int px = 0; px < 16; px++)
        {
            const unsigned sel = (bestSelectors >> (px * 2)) & 3;
            sectorBits |= remapSector[sel] << px;
            signBits |= remapSign[sel] << px;
        }
        const int blockColors[2] = {bestLineColor, bestHColor2};
        etc2_emit_h(ln->out, blockColors, sectorBits, signBits, bestTable, 0);
    }
    else
    {
        int lineColor[3];
        for (int ch = 0; ch < 3; ch++)
            lineColor[ch] = (bestLineColor >> (10 - ch * 5)) & 15;
        etc2_emit_t(ln->out, lineColor, vs->isoQ, bestSelectors, bestTable, 0);
    }
}

/* ---- punch-through: CompressETC1PunchthroughBlockInternal, ETC.cpp:2885-3082, TestHalfBlockPunchthrough 151-217 ----
 * Restated with its quirks: the per-half count the base colours are divided by is the number of TRANSPARENT pixels
 * (2949-2951), and only half 0 can be "ignored" (canIgnoreSector starts as {true, false}, 2938). */
static void etc1_punchthrough(const etc_ctx_t *cx, etc_lane_t *ln)
{
    static __thread etc_attempt_t attempts[2][160];
    static __thread uint16_t sortIdx[2][160];
    int bestIsThisMode = 0, bestFlip = 0, bestTables[2] = {0, 0};
    unsigned bestColors[2] = {0, 0}, bestSelectors[2] = {0, 0};
    for (int flip = 0; flip < 2; flip++)
    {
        int numAttempts[2] = {0, 0};
        int canIgnore0 = 1;
        for (int px = 0; px < 8; px++)
            canIgnore0 = canIgnore0 && ln->transparent[etc_flip_tables[flip][0][px]];
        for (int sector = 0; sector < 2; sector++)
        {
            int cumulative[3] = {0, 0, 0}, spix[8][3], strans[8], count = 0;
            float spw[8][3];
            for (int px = 0; px < 8; px++)
            {
                const int src = etc_flip_tables[flip][sector][px];
                for (int ch = 0; ch < 3; ch++)
                {
                    spix[px][ch] = ln->pixels[src][ch];
                    spw[px][ch] = ln->pw[src][ch];
                    cumulative[ch] += spix[px][ch];
                }
                strans[px] = ln->transparent[src];
                count += strans[px];
            }
            const int denominator = (count > 1 ? count : 1) << 8, addend = count << 7, cumulativeMax = 255 * count;
            for (int table = 0; table < 8; table++)
            {
                const int modifier = orc_etc1_modifiers[table * 4 + 3]; /* 8, 17, 29, 42, 60, 80, 106, 183 */
                unsigned colors[17];
                int n = 0;
                for (int om = -count; om <= count; om++)
                {
                    const int offset = (int16_t)(om * modifier);
                    unsigned packed = 0;
                    for (int ch = 0; ch < 3; ch++)
                    {
                        int cu = (int16_t)(cumulative[ch] + offset);
                        if (cu < 0) cu = 0;
                        if (cu > cumulativeMax) cu = cumulativeMax;
                        const unsigned numerator = ((((unsigned)cu << 5) - (unsigned)cu) + (((unsigned)cu >> 3) + (unsigned)addend)) & 0xffffu;
                        packed |= (numerator / (unsigned)denominator) << (ch * 5);
                    }
                    if (n == 0 || packed != colors[n - 1])
                        colors[n++] = packed;
                }
                for (int i = 0; i < n; i++)
                {
                    int modified[3][3];
                    for (int ch = 0; ch < 3; ch++)
                    {
                        const int q = (colors[i] >> (ch * 5)) & 31;
                        const int u = (q << 3) | (q >> 2);
                        modified[0][ch] = (u > modifier ? u : modifier) - modifier;
                        modified[1][ch] = u;
                        modified[2][ch] = u + modifier < 255 ? u + modifier : 255;
                    }
                    unsigned selectors = 0;
                    float totalError = 0.0f;
                    for (int px = 0; px < 8; px++)
                    {
                        float bestError = FLT_MAX;
                        unsigned bestSelector = 0;
                        for (unsigned sl = 0; sl < 3; sl++)
                        {
                            const float e = etc_error(cx, modified[sl], spix[px], spw[px]);
                            if (e < bestError) bestSelector = sl;
                            bestError = f_min(e, bestError);
                        }
                        bestSelector = bestSelector << 1 < 3 ? bestSelector << 1 : 3; /* 0, 2, 3: index 1 is "transparent" */
                        if (strans[px])
                        {
                            bestError = 0.0f;
                            bestSelector = 1;
                        }
                        totalError = totalError + bestError;
                        selectors |= bestSelector << (px * 2);
                    }
                    etc_attempt_t *a = &attempts[sector][numAttempts[sector]++];
                    a->error = totalError;
                    a->selectors = (uint16_t)selectors;
                    a->color = (uint16_t)colors[i];
                    a->table = (uint8_t)table;
                }
            }
        }

        /* FindBestDifferentialCombination(flip, 1, canIgnoreSector = {canIgnore0, false}), ETC.cpp:219-362 */
        float blockBest = ln->bestError;
        float bestDiffErrors[2] = {FLT_MAX, FLT_MAX};
        int bestAttempt[2] = {0, 0};
        for (int sector = 0; sector < 2; sector++)
            for (int i = 0; i < numAttempts[sector]; i++)
                if (attempts[sector][i].error < bestDiffErrors[sector])
                {
                    bestDiffErrors[sector] = attempts[sector][i].error;
                    bestAttempt[sector] = i;
                }
        if (!(bestDiffErrors[0] + bestDiffErrors[1] < blockBest))
            continue;
        const etc_attempt_t *a0 = &attempts[0][bestAttempt[0]], *a1 = &attempts[1][bestAttempt[1]];
        if (canIgnore0 || etc_diff_legal(a0->color, a1->color))
        {
            bestIsThisMode = 1;
            ln->bestError = bestDiffErrors[0] + bestDiffErrors[1];
            bestFlip = flip;
            bestColors[0] = canIgnore0 ? a1->color : a0->color;
            bestColors[1] = a1->color;
            bestSelectors[0] = a0->selectors; bestSelectors[1] = a1->selectors;
            bestTables[0] = a0->table; bestTables[1] = a1->table;
            continue;
        }
        int numSort[2] = {0, 0};
        for (int sector = 0; sector < 2; sector++)
        {
            for (int i = 0; i < numAttempts[sector]; i++)
                if (attempts[sector][i].error < blockBest)
                    sortIdx[sector][numSort[sector]++] = (uint16_t)i;
            for (int i = 1; i < numSort[sector]; i++)
            {
                uint16_t key = sortIdx[sector][i];
                float ke = attempts[sector][key].error;
                int j = i - 1;
                while (j >= 0)
                {
                    uint16_t o = sortIdx[sector][j];
                    float oe = attempts[sector][o].error;
                    if (oe < ke || (!(oe > ke) && o < key))
                        break;
                    sortIdx[sector][j + 1] = o;
                    j--;
                }
                sortIdx[sector][j + 1] = key;
            }
        }
        for (int i = 0; i < numSort[0]; i++)
        {
            const etc_attempt_t *a0s = &attempts[0][sortIdx[0][i]];
            const float error0 = a0s->error;
            if (error0 >= blockBest)
                break;
            const float maxError1 = ln->bestError - error0;
            if (maxError1 < bestDiffErrors[1])
                break;
            for (int j = 0; j < numSort[1]; j++)
            {
                const etc_attempt_t *a1s = &attempts[1][sortIdx[1][j]];
                if (a1s->error >= maxError1)
                    break;
                if (etc_diff_legal(a0s->color, a1s->color))
                {
                    blockBest = error0 + a1s->error;
                    bestIsThisMode = 1;
                    ln->bestError = blockBest;
                    bestFlip = flip;
                    bestColors[0] = a0s->color; bestColors[1] = a1s->color;
                    bestSelectors[0] = a0s->selectors; bestSelectors[1] = a1s->selectors;
                    bestTables[0] = a0s->table; bestTables[1] = a1s->table;
                    break;
                }
            }
        }
    }
    if (!bestIsThisMode)
        return;
    /* EmitETC1Block(d = 1, transparent = true): differential layout with the opaque bit left clear */
    int colors[2][3];
    for (int sc = 0; sc < 2; sc++)
        for (int ch = 0; ch < 3; ch++)
            colors[sc][ch] = (bestColors[sc] >> (ch * 5)) & 31;
    uint32_t highBits = 0, lowBits = 0;
    highBits |= (uint32_t)colors[0][0] << 27;
    highBits |= (uint32_t)((colors[1][0] - colors[0][0]) & 7) << 24;
    highBits |= (uint32_t)colors[0][1] << 19;
    highBits |= (uint32_t)((colors[1][1] - colors[0][1]) & 7) << 16;
    highBits |= (uint32_t)colors[0][2] << 11;
    highBits |= (uint32_t)((colors[1][2] - colors[0][2]) & 7) << 8;
    highBits |= (uint32_t)bestTables[0] << 5;
    highBits |= (uint32_t)bestTables[1] << 2;
    highBits |= (uint32_t)bestFlip;
    static const uint8_t modifierCodes[4] = {3, 2, 0, 1};
    uint8_t codes[16];
    for (int sector = 0; sector < 2; sector++)
        for (int px = 0; px < 8; px++)
            codes[etc_flip_tables[bestFlip][sector][px]] = modifierCodes[(bestSelectors[sector] >> (2 * px)) & 3];
    for (int sb = 0; sb < 2; sb++)
        for (int px = 0; px < 16; px++)
            lowBits |= (uint32_t)((codes[etc_selector_order[px]] >> sb) & 1) << (px + sb * 16);
    put_be32(ln->out, highBits);
    put_be32(ln->out + 4, lowBits);
}

/* CompressETC2Block for one group, ETC.cpp:1664-1887 (cx->punchthrough selects EncodeETC2PunchthroughAlpha).
 * err: NULL, or 8 floats that receive each block's final bestError, the score of the candidate that is emitted. */
static void etc2_encode_group_color(const uint8_t *blocks, uint8_t *out, size_t outStride, const etc_ctx_t *cx, float *err,
                                    uint32_t siteMask, int siteLane)
{
    static __thread etc_lane_t lanes[8];
    int groupAny = 0, groupAll = 1; /* AnySet(anyTransparent), AllSet(allTransparent) */
    for (int l = 0; l < 8; l++)
    {
        etc_lane_t *ln = &lanes[l];
        ln->anyTransparent = 0;
        ln->allTransparent = 1;
        ln->numOpaque = 16;
        for (int px = 0; px < 16; px++)
        {
            ln->transparent[px] = cx->punchthrough && blocks[l * 64 + px * 4 + 3] < cx->alphaThreshold;
            ln->anyTransparent |= ln->transparent[px];
            ln->allTransparent &= ln->transparent[px];
            ln->numOpaque -= ln->transparent[px];
        }
        if (!cx->punchthrough)
            ln->allTransparent = 0;
        groupAny |= ln->anyTransparent;
        groupAll &= ln->allTransparent;
    }
    if (siteMask & ORC_SITE_ETC2_PUNCH_ALPHA)
    {
        /* site switch: AnySet / AllSet answered by the viewing lane's own flags */
        groupAny = lanes[siteLane].anyTransparent;
        groupAll = lanes[siteLane].allTransparent;
    }
    for (int l = 0; l < 8; l++)
    {
        etc_lane_t *ln = &lanes[l];
        for (int px = 0; px < 16; px++)
            for (int ch = 0; ch < 3; ch++)
            {
                ln->pixels[px][ch] = blocks[l * 64 + px * 4 + ch];
                float f = (float)ln->pixels[px][ch];
                if (cx->uniform)
                    ln->pw[px][ch] = f;
                else
                    ln->pw[px][ch] = f * (ch == 0 ? cx->rw : (ch == 1 ? cx->gw : cx->bw));
            }
        if (cx->fake) /* ExtractBlocks, ETC.cpp:2141-2142: takes precedence over Uniform */
            for (int px = 0; px < 16; px++)
                etc_to_fake709(ln->pw[px], (float)ln->pixels[px][0], (float)ln->pixels[px][1], (float)ln->pixels[px][2]);
        for (int px = 0; px < 16; px++)
            if (ln->transparent[px]) /* ETC.cpp:1706-1720 */
                for (int ch = 0; ch < 3; ch++)
                {
                    ln->pixels[px][ch] = 0;
                    ln->pw[px][ch] = 0.0f;
                }
        ln->bestError = FLT_MAX;
        memset(ln->out, 0, 8);
        if (!groupAll)
            etc2_planar(cx, ln);
        etc2_sector_assignments(cx, ln);
    }
    /* T mode needs the group-wide maximum of the per-lane unique colour counts (hazard H2) */
    for (int call = 0; call < 2 && !groupAll; call++)
    {
        int gmax[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int flags[8][16];
        for (int l = 0; l < 8; l++)
        {
            for (int px = 0; px < 16; px++)
                flags[l][px] = call == 0 ? lanes[l].isolated[px] : !lanes[l].isolated[px];
            tmode_setup_t ts;
            tmode_setup(cx, &lanes[l], flags[l], &ts);
            for (int table = 0; table < 8; table++)
            {
                int colors[40];
                int n = tmode_unique(cx, &ts, table, colors);
                /* site switch: the viewing lane's own count in place of the group maximum (slot H2 is then never read) */
                if ((siteMask & ORC_SITE_ETC2_OPAQUE_TMAX) && l != siteLane) continue;
                if (n > gmax[table]) gmax[table] = n;
            }
        }
        for (int l = 0; l < 8; l++)
            etc2_tmode(cx, &lanes[l], flags[l], gmax);
        if (call == 1)
            for (int l = 0; l < 8; l++)
            {
                etc2_hmode(cx, &lanes[l], flags[l]);
                etc1_cluster_fit(cx, &lanes[l], 1);
            }
    }
    if (groupAny)
    {
        /* ETC.cpp:1865-1886: blocks with a transparent pixel start over; EVERY block of the group goes through the
         * punch-through modes (an opaque block keeps its opaque result unless one of them is strictly better) */
        for (int l = 0; l < 8; l++)
            if (lanes[l].anyTransparent)
                lanes[l].bestError = FLT_MAX;
        for (int call = 0; call < 2; call++)
        {
            int flags[8][16], clusterMaxLine = 0, gmax[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            static __thread vt_setup_t vs[8];
            for (int l = 0; l < 8; l++)
            {
                for (int px = 0; px < 16; px++)
                    flags[l][px] = call == 0 ? lanes[l].isolated[px] : !lanes[l].isolated[px];
                vt_setup(cx, &lanes[l], flags[l], &vs[l]);
                if (vs[l].numLine > clusterMaxLine) clusterMaxLine = vs[l].numLine;
            }
            /* site switch: the viewing lane's own line count and unique-colour counts in place of the group maxima */
            if (siteMask & ORC_SITE_ETC2_PUNCH_TMAX)
                clusterMaxLine = vs[siteLane].numLine;
            for (int l = 0; l < 8; l++)
                for (int table = 0; table < 8; table++)
                {
                    int colors[40];
                    int n = vt_unique(cx, &vs[l], table, clusterMaxLine, colors);
                    if ((siteMask & ORC_SITE_ETC2_PUNCH_TMAX) && l != siteLane) continue;
                    if (n > gmax[table]) gmax[table] = n;
                }
            for (int l = 0; l < 8; l++)
                etc2_virtual_tmode(cx, &lanes[l], &vs[l], clusterMaxLine, gmax);
        }
        for (int l = 0; l < 8; l++)
            etc1_punchthrough(cx, &lanes[l]);
    }
    for (int l = 0; l < 8; l++)
        memcpy(out + l * outStride, lanes[l].out, 8);
    if (err)
        for (int l = 0; l < 8; l++)
            err[l] = lanes[l].bestError;
}

/* CompressETC1Block, ETC.cpp:2116-2126: lanes are independent (the group-wide padding of the candidate lists only
 * repeats a colour already tried, and repeats never pass the strict '<') */
static void etc1_encode_group(const uint8_t *blocks, uint8_t *out, const etc_ctx_t *cx, float *err)
{
    static __thread etc_lane_t lane;
    for (int l = 0; l < 8; l++)
    {
        etc_lane_t *ln = &lane;
        for (int px = 0; px < 16; px++)
            for (int ch = 0; ch < 3; ch++)
            {
                ln->pixels[px][ch] = blocks[l * 64 + px * 4 + ch];
                float f = (float)ln->pixels[px][ch];
                ln->pw[px][ch] = cx->uniform ? f : f * (ch == 0 ? cx->rw : (ch == 1 ? cx->gw : cx->bw));
            }
        if (cx->fake)
            for (int px = 0; px < 16; px++)
                etc_to_fake709(ln->pw[px], (float)ln->pixels[px][0], (float)ln->pixels[px][1], (float)ln->pixels[px][2]);
        ln->bestError = FLT_MAX;
        memset(ln->out, 0, 8);
        etc1_cluster_fit(cx, ln, 0);
        memcpy(out + l * 8, ln->out, 8);
        if (err)
            err[l] = ln->bestError;
    }
}

typedef struct
{
    etc_ctx_t cx;
    int mode;
    uint32_t siteMask;  /* group-coupling site switch (cvtt_oracle.h) */
    float *colorErr;    /* NULL, or one float per block (modes 0, 1, 3, 4) */
    uint32_t *alphaErr; /* NULL, or one uint32 per block (modes 1, 2) */
} etc_job_t;

#define ETC2_SITES (ORC_SITE_ETC2_OPAQUE_TMAX | ORC_SITE_ETC2_PUNCH_TMAX | ORC_SITE_ETC2_PUNCH_ALPHA)

static void etc2_group_thunk(const uint8_t *in, uint8_t *out, const void *a, const void *b, const float *rcp, size_t group)
{
    (void)b;
    (void)rcp;
    const etc_job_t *job = (const etc_job_t *)a;
    float *cerr = job->colorErr ? job->colorErr + group * 8 : NULL;
    uint32_t *aerr = job->alphaErr ? job->alphaErr + group * 8 : NULL;
    if (job->mode == 0 || job->mode == 4)
        ORC_RUN_SITED(job->siteMask, ETC2_SITES, out, 8, 8,
                      etc2_encode_group_color(in, sitedOut, 8, &job->cx, sitedMask ? NULL : cerr, sitedMask, siteLane));
    else if (job->mode == 3)
        etc1_encode_group(in, out, &job->cx, cerr);
    else if (job->mode == 1)
    {
        /* EncodeETC2RGBA, API.cpp:270-286: [alpha 8 B | colour 8 B] */
        ORC_RUN_SITED(job->siteMask, ETC2_SITES, out + 8, 16, 8,
                      etc2_encode_group_color(in, sitedOut, 16, &job->cx, sitedMask ? NULL : cerr, sitedMask, siteLane));
        for (int l = 0; l < 8; l++)
            etc2_alpha_block(in + l * 64, out + l * 16, aerr ? aerr + l : NULL);
    }
    else
        for (int l = 0; l < 8; l++)
            etc2_alpha_block(in + l * 64, out + l * 8, aerr ? aerr + l : NULL);
}

int orc_encode_etc2(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, int mode, int threads)
{
    return orc_encode_etc2_alloc(out, blocks, numBlocks, options, options, mode, threads);
}

/* allocOptions: the Options AllocETC2Data was called with; the two chroma axes are computed from ITS colour weights when the
 * scratch is constructed (ETC.cpp:3117-3145), everything else comes from the Options of the Encode call */
static int etc2_encode(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, const orc_options *allocOptions,
                       int mode, int threads, float *colorErr, uint32_t *alphaErr, uint32_t siteMask)
{
    if (numBlocks % 8 != 0 || mode < 0 || mode > 4) /* 3 = ETC1 (EncodeETC1, API.cpp:201-214), 4 = EncodeETC2PunchthroughAlpha (231-244) */
        return -1;
    etc_job_t job;
    job.mode = mode;
    job.siteMask = siteMask;
    job.colorErr = mode == 2 ? NULL : colorErr;
    job.alphaErr = (mode == 1 || mode == 2) ? alphaErr : NULL;
    job.cx.flags = options->flags;
    job.cx.uniform = (options->flags & ORC_FLAG_UNIFORM) != 0;
    job.cx.fake = (options->flags & 0x400u) != 0;
    job.cx.fakeAccurate = (options->flags & 0x800u) != 0;
    job.cx.rw = options->redWeight;
    job.cx.gw = options->greenWeight;
    job.cx.bw = options->blueWeight;
    etc2_chroma_axes(allocOptions ? allocOptions : options, job.cx.axis0, job.cx.axis1);
    job.cx.punchthrough = mode == 4;
    {
        float t = options->threshold;
        t = (1.0f < t ? 1.0f : t);
        t = (t > 0.0f ? t : 0.0f); /* std::max(std::min(1.0f, threshold), 0.0f) */
        job.cx.alphaThreshold = (int)(uint16_t)floorf(t * 255.0f + 1.0f);
    }
    const size_t outPer = mode == 1 ? 16 : 8;
    run_groups(etc2_group_thunk, blocks, out, numBlocks / 8, 8 * 64, 8 * outPer, &job, NULL, NULL, threads);
    return 0;
}

int orc_encode_etc2_alloc(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, const orc_options *allocOptions,
                          int mode, int threads)
{
    return etc2_encode(out, blocks, numBlocks, options, allocOptions, mode, threads, NULL, NULL, 0);
}

int orc_encode_etc2_sites(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, const orc_options *allocOptions,
                          int mode, int threads, uint32_t siteMask)
{
    return etc2_encode(out, blocks, numBlocks, options, allocOptions, mode, threads, NULL, NULL, siteMask);
}
