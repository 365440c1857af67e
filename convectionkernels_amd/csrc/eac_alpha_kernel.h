// EAC alpha: the integer-only, lane-independent search for 8-bit alpha and 11-bit R11 blocks (cvttmi_eac_alpha_kernel), the
// launch-size threshold between its two lane mappings.  Part of etc2_kernel.hip (one translation unit, one object, one flag
// set), included behind the colour kernel; both launchers stay there.
#pragma once

// EAC 8-bit alpha: CompressETC2AlphaBlockInternal (ETC.cpp:1902-2085), QuantizeETC2Alpha 2366-2411.
// KIND 0: 8-bit alpha of PixelBlockU8 (EncodeETC2Alpha / the alpha half of EncodeETC2RGBA);
// KIND 1 / 2: unsigned / signed 11-bit EAC of PixelBlockScalarS16 (EncodeETC2Alpha11, CompressEACBlock ETC.cpp:2087-2114)
// SPREAD = false: one lane per block (the throughput form: a wave's 64 blocks share every table word).
// SPREAD = true: sixteen lanes per block, lane t searches modifier table t, and a 16-lane minimum of (error, table) picks the
// winner -- the reference walks the tables in ascending order and keeps the first minimum, i.e. the lowest table among equal
// errors.  The same instructions per block, but a sixteenth of the latency: what a call with a handful of blocks (the
// reference's 8-block convention, ConvectionKernels_API.cpp:246-256, 270-286) waits for (213 -> 25 us at 16 blocks).
template <int KIND, bool SPREAD>
__global__ __launch_bounds__(64) void cvttmi_eac_alpha_kernel(const uint8_t *__restrict__ blocks, uint8_t *__restrict__ out,
                                                             const CvttEtcArgs A, const CvttDeviceTables *__restrict__ T)
{
    constexpr bool is11 = KIND != 0, isSigned = KIND == 2;
    const u32 blockIndex = SPREAD ? blockIdx.x * 4u + (threadIdx.x >> 4) : blockIdx.x * 64u + threadIdx.x;
    const bool valid = blockIndex < A.numBlocks;
    int pixel[16];
    if (!is11)
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(blocks + (size_t)(valid ? blockIndex : 0u) * 64u);
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const uint4 v = src[i];
            pixel[4 * i + 0] = (int)(v.x >> 24);
            pixel[4 * i + 1] = (int)(v.y >> 24);
            pixel[4 * i + 2] = (int)(v.z >> 24);
            pixel[4 * i + 3] = (int)(v.w >> 24);
        }
    }
    else
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(blocks + (size_t)(valid ? blockIndex : 0u) * 32u);
#pragma unroll
        for (int i = 0; i < 2; i++)
        {
            const uint4 v = src[i];
            const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 8; j++)
            {
                int x = (int)(short)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
                // shifted ranges: signed 1..2047, unsigned 0..2047
                if (isSigned)
                {
                    x = (x > 1023 ? 1023 : x) + 1024;
                    x = x < 1 ? 1 : x;
                }
                else
                    x = x > 2047 ? 2047 : (x < 0 ? 0 : x);
                pixel[8 * i + j] = x;
            }
        }
    }
    int minAlpha = is11 ? 2047 : 255, maxAlpha = 0;
#pragma unroll
    for (int px = 0; px < 16; px++)
    {
        minAlpha = pixel[px] < minAlpha ? pixel[px] : minAlpha;
        maxAlpha = pixel[px] > maxAlpha ? pixel[px] : maxAlpha;
    }
    const int alphaSpan = maxAlpha - minAlpha;
    const int midTimes2 = maxAlpha + minAlpha;

    u32 bestTotalError = 0x7fffffffu;
    int bestTable = 0, bestBase = 0, bestMultiplier = 0;
    u32 bestIdxLo = 0, bestIdxHi = 0; // 3 bits per pixel

    for (int tableIter = 0; tableIter < (SPREAD ? 1 : 16); tableIter++)
    {
        const int tableIndex = SPREAD ? (int)(threadIdx.x & 15u) : tableIter;
        const int pos[4] = {T->eacPositive[tableIndex][0], T->eacPositive[tableIndex][1], T->eacPositive[tableIndex][2], T->eacPositive[tableIndex][3]};
        // the table's row of the rounding table (13 entries of 2 bits) and its four positive modifiers as two wave-uniform
        // words: a pixel's lookups are bit-field extracts instead of a per-lane byte load and a select chain
        u32 roundBits = 0;
        for (int i = 0; i < 13; i++)
            roundBits |= (u32)T->eacRounding[tableIndex][i] << (2 * i);
        u32 posWord = (u32)(pos[0] | (pos[1] << 8) | (pos[2] << 16) | (pos[3] << 24));
        if (!SPREAD)
        {
            roundBits = (u32)__builtin_amdgcn_readfirstlane((int)roundBits);
            posWord = (u32)__builtin_amdgcn_readfirstlane((int)posWord);
        }
        for (int r = 0; r < 10; r++)
        {
            const int subrange = r % 3, mainRange = r / 3;
            const int maxOffset = T->eacPositive[tableIndex][3 - mainRange - (subrange & 1)];
            const int minOffset = -(int)T->eacPositive[tableIndex][3 - mainRange - ((subrange >> 1) & 1)] - 1;
            const int offsetSpan = maxOffset - minOffset;
            int minMultiplier = udivSmall(alphaSpan, offsetSpan);
            if (is11)
            {
                minMultiplier = minMultiplier > 112 ? 112 : minMultiplier;
                minMultiplier &= 120;
            }
            else
            {
                minMultiplier = minMultiplier > 14 ? 14 : minMultiplier;
                minMultiplier = minMultiplier < 1 ? 1 : minMultiplier;
            }
            for (int mo = 0; mo < 2; mo++)
            {
                int multiplier = minMultiplier;
                if (is11)
                {
                    if (mo == 1)
                        multiplier += 8;
                    else
                        multiplier = multiplier < 1 ? 1 : multiplier;
                }
                else
                    multiplier += mo;
                int base2 = midTimes2 - multiplier * maxOffset - multiplier * minOffset; // all lanes stay inside 16 bits
                int baseAlpha;
                if (is11)
                {
                    if (isSigned)
                        base2 += 8;
                    const int lo2 = isSigned ? 16 : 0;
                    base2 = base2 < lo2 ? lo2 : (base2 > 4095 ? 4095 : base2);
                    baseAlpha = (base2 >> 1) & 2040;
                    if (!isSigned)
                        baseAlpha += 4;
                }
                else
                {
                    base2 = base2 < 0 ? 0 : (base2 > 510 ? 510 : base2);
                    baseAlpha = (base2 + 1) >> 1;
                }
                // lookup / multiplier for lookup < 2^12, multiplier <= 128: (lookup * ceil(2^20 / multiplier)) >> 20 is exact
                // (the excess of the magic number adds less than lookup / 2^20 < 1/256 to a quotient whose fraction is at most
                // 127/128), one 24-bit multiply and a shift per pixel; the magic number is per candidate
                const u32 magic = (u32)udivSmall20(multiplier);
                u32 totalError = 0; // (only the error: the winner's indexes are worked out again after the search)
#pragma unroll
                for (int px = 0; px < 16; px++)
                {
                    const int a = pixel[px];
                    const int refl2 = (a - baseAlpha) * 2 + multiplier;
                    const int absv = refl2 < 0 ? -refl2 : refl2;
                    const int lookup = absv >> 1;
                    int li = (int)(__umul24((u32)lookup, magic) >> 20);
                    li = li >= 13 ? 12 : li;
                    const int index = (int)((roundBits >> (2 * li)) & 3u);
                    const int pOff = (int)((posWord >> (8 * index)) & 0xffu);
                    const int sign = refl2 < 0 ? -1 : 0;
                    const int quantizedOffset = (pOff ^ sign) * multiplier;
                    int q = baseAlpha + quantizedOffset;
                    const int qLo = (is11 && isSigned) ? 1 : 0, qHi = is11 ? 2047 : 255;
                    q = q < qLo ? qLo : (q > qHi ? qHi : q);
                    const int d = q - a;
                    totalError += (u32)(d * d);
                }
                if (totalError < bestTotalError)
                {
                    bestTotalError = totalError;
                    bestTable = tableIndex;
                    bestBase = baseAlpha;
                    bestMultiplier = multiplier;
                }
            }
        }
    }
    if (SPREAD)
    {
        // (error, table) as one word: the error of 16 pixels stays below 2^27 (16 x 2047^2)
        u32 key = (bestTotalError << 4) | (u32)bestTable;
#pragma unroll
        for (int step = 1; step < 16; step <<= 1)
        {
            const u32 o = (u32)__shfl_xor((int)key, step);
            key = o < key ? o : key;
        }
        const int src = (int)((threadIdx.x & ~15u) | (key & 15u));
        bestTable = (int)(key & 15u);
        bestBase = __shfl(bestBase, src);
        bestMultiplier = __shfl(bestMultiplier, src);
    }
    // the winner's indexes (the operations of the candidate loop, once)
    {
        const u32 magic = (u32)udivSmall20(bestMultiplier);
#pragma unroll
        for (int px = 0; px < 16; px++)
        {
            const int refl2 = (pixel[px] - bestBase) * 2 + bestMultiplier;
            const int absv = refl2 < 0 ? -refl2 : refl2;
            int li = (int)(__umul24((u32)(absv >> 1), magic) >> 20);
            li = li >= 13 ? 12 : li;
            const int index = T->eacRounding[bestTable][li];
            const u32 code = (u32)(index + 4 - ((refl2 < 0 ? -1 : 0) & 4));
            if (px < 8)
                bestIdxLo |= code << (3 * px);
            else
                bestIdxHi |= code << (3 * (px - 8));
        }
    }
    if (is11)
    {
        bestMultiplier >>= 3;
        if (isSigned)
            bestBase ^= 0x80;
    }
    if (valid && (!SPREAD || (threadIdx.x & 15u) == 0))
    {
        // 16 x 3-bit indexes, column-major pixel order, MSB first (ETC.cpp:2049-2084)
        u64 bits = 0;
#pragma unroll
        for (int s = 0; s < 16; s++)
        {
            const int px = ((s & 3) << 2) | (s >> 2); // s-th emitted = pixel with selectorOrder[px] == s
            const u32 code = px < 8 ? (bestIdxLo >> (3 * px)) & 7u : (bestIdxHi >> (3 * (px - 8))) & 7u;
            bits = (bits << 3) | code;
        }
        uint8_t *o = out + (size_t)blockIndex * A.outStride + A.outOffset;
        const u32 w0 = ((u32)bestBase & 0xffu) | ((u32)(((bestMultiplier << 4) | bestTable) & 0xff) << 8) | ((u32)((bits >> 40) & 0xff) << 16) | ((u32)((bits >> 32) & 0xff) << 24);
        const u32 w1 = bswap32((u32)bits);
        uint2 v;
        v.x = w0;
        v.y = w1;
        *reinterpret_cast<uint2 *>(o) = v;
    }
}

// Launches of at most this many blocks use the sixteen-lanes-per-block form of the EAC search: the chip is not full there
// (256 CUs x 4 SIMDs x 4 waves x 64 lanes = 262 144 blocks resident in the one-lane form), so latency is what counts.
static const uint32_t kEacSpreadMax = 65536u;
