// BC7 single-plane chains and what the search shares: end-point quantisation, the modes' static description, the
// order-preserving argmins, one chain of a single-plane shape (evalChain), the PCA seeds of a block staged in LDS, the
// records the phases of the search hand each other, and the packer of the dual-plane modes.
// Part of bc7_kernel.hip (one translation unit), included after its tuning knobs and PROF_* macros.
#pragma once

namespace
{
// ---- BC7 endpoint quantisation (reference BC67.cpp:829-860); all values fit 16 bits ----
__device__ __forceinline__ int quantizeNoP(int v, int bits) { return ((v << bits) - v + (127 + (1 << (7 - bits)))) >> 8; }
__device__ __forceinline__ int quantizeP(int v, int bits, int p)
{
    const int addend = p ? ((1 << (8 - bits)) - 1) : 255;
    const int q = ((v << (bits + 1)) - v + addend) >> 9;
    return (q << 1) | p;
}
__device__ __forceinline__ int unquantize(int v, int bits)
{
    const int t = v << (8 - bits);
    return t | (t >> bits);
}

// Static description of a single-plane mode (BC7 format + reference BC67.cpp:862-938).
struct ModeDesc
{
    int mode;
    int indexBits;
    int numP;     // parity combinations: 4 per-endpoint, 2 per-subset, 1 none
    int quantBits;
    int unquantBits; // 0 = value is already 8 bit
};

__device__ __forceinline__ void compressEndpoints(const ModeDesc &md, int (&ep)[2][4], int pIter, bool isRGB)
{
    const int nch = isRGB ? 3 : 4;
#pragma unroll
    for (int j = 0; j < 2; j++)
    {
        // p-bit of endpoint j: per-endpoint modes use bit j of pIter, per-subset modes share
        // bit 0 (reference BC67.cpp:1307-1309, 872-880)
        const int p = (md.numP == 4) ? ((pIter >> j) & 1) : (pIter & 1);
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
        {
            if (ch < nch)
            {
                int v = ep[j][ch];
                v = (md.numP == 1) ? quantizeNoP(v, md.quantBits) : quantizeP(v, md.quantBits, p);
                if (md.unquantBits)
                    v = unquantize(v, md.unquantBits);
                ep[j][ch] = v;
            }
        }
        if (isRGB)
            ep[j][3] = 255;
    }
}

struct ShapeBest
{
    float err;
    u32 ep0, ep1; // packed RGBA endpoints
    u32 idxLo, idxHi; // 4 bits per pixel: compact by member (evalChain), or by dualIndexSlot (evalDual)
};

// The index sets of a dual-plane candidate (ShapeBest::idxLo / idxHi out of evalDual, WorkState::idxLo .. idx2Hi, s_parked)
// keep the layout the pixel loop of the search produces them in: idxLo holds pixels 0..7, idxHi pixels 8..15, and pixel p
// sits in the 4-bit slot dualIndexSlot(p) of its word -- byte k of a word holds pixel k of the even group of four in its low
// nibble and pixel k of the odd group in its high nibble, which is one v_lshl_or_b32 per pair of groups from the bytes that
// v_cvt_pk_u8_f32 files.  Pixel 0 stays in slot 0.  packDualPlane reads every pixel from its slot: the sets are sorted to
// their pixels once per block, where the bits are written, instead of in every round that improves a plane.
__device__ __forceinline__ constexpr int dualIndexSlot(int p) { return 2 * (p & 3) + ((p >> 2) & 1); }

__device__ __forceinline__ u32 packEP(const int (&e)[4])
{
    return (u32)e[0] | ((u32)e[1] << 8) | ((u32)e[2] << 16) | ((u32)e[3] << 24);
}

// Order-preserving argmin over the 4 lanes of a quad; ties go to the lower sub-lane, which
// is the earlier candidate in the reference's sequential commit order.
__device__ __forceinline__ void quadArgminBroadcast(ShapeBest &b, int lane)
{
    int who = lane & 3;
    float err = b.err;
#pragma unroll
    for (int step = 1; step <= 2; step <<= 1)
    {
        const float oErr = xorLane(err, step);
        const int oWho = xorLane(who, step);
        const bool take = (oErr < err) || (oErr == err && oWho < who);
        err = take ? oErr : err;
        who = take ? oWho : who;
    }
    const int src = (lane & ~3) | who;
    b.err = err;
    b.ep0 = __shfl(b.ep0, src);
    b.ep1 = __shfl(b.ep1, src);
    b.idxLo = __shfl(b.idxLo, src);
    b.idxHi = __shfl(b.idxHi, src);
}

// One CHAIN of a single-plane shape: a (p-bit combination, seed point) pair of the reference's
// pIter x tweak loops (BC67.cpp:1298-1434) with its refine rounds, run by one lane.  The
// pixels of the block are read from LDS (`lp`, 16 packed RGBA8 words) in ascending order of
// the shape's members.  NRC = numRealChannels (3 for modes 0-3).  maxCount = wave-uniform
// upper bound on popcount(mask).
// TRACE (BC7_RespectPunchThrough only): every round's error is also written to trialErr[round], and with
// captureRound >= 0 the result is that round's instead of the best one.
// `list`: the member pixels in ascending order, 4 bits each (UnitRec::listLo / listHi); best.idxLo / idxHi come back COMPACT: the
// index of member i in bits [4i, 4i + 4) (expandIndexes puts them at their pixel positions when a block is packed).
// wantPayload (wave-uniform) = false: only best.err is wanted (probes).
// A chain cut into pieces (the probes run round 0 of every chain first and the later rounds only once per distinct set of
// end points): rounds [firstRound, endRound) are run.  firstRound > 0: ep0 / ep1 bring that round's (compressed) end points.
// endRound < numRefine: ep0 / ep1 take the compressed end points of round endRound away.  r0ep0 / r0ep1: the compressed
// end points the first executed round used.  (Wave-uniform except for the end points.)
struct ChainSplit
{
    int firstRound, endRound;
    u32 ep0, ep1;
    u32 r0ep0, r0ep1;
};

template <int NRC, bool FAST, bool TRACE>
__device__ __forceinline__ void evalChain(const u32 *lp, u32 mask, u64 list, int maxCount, const ModeDesc md, const Unfinished &u,
                                          int pIter, int tweak, bool active, const CvttBc7Args &A,
                                          const CvttDeviceTables *__restrict__ T, int numRefine, ShapeBest &best,
                                          const float (&vs)[4], bool wantPayload = true, float *trialErr = nullptr, int captureRound = -1, float *trialErrHbm = nullptr,
                                          ChainSplit *split = nullptr)
{
    const bool isRGB = (NRC == 3);
    const int range = 1 << md.indexBits;
    // (literals: the clamp below then needs no canonicalising v_max_f32 per pixel)
    const float maxValue = md.indexBits == 2 ? 3.0f : md.indexBits == 3 ? 7.0f : 15.0f;
    const float rcpMaxIndex = T->rcpMaxIndex[md.indexBits];
    const int weightRcp = (65536 + (range - 1)) / (2 * (range - 1)); // g_weightReciprocals, IndexSelector.cpp:43-62
    const int count = __popc(mask);
    const float wRcp = T->rcpTable[count];
    const float wCount = (float)count;
    const bool uniformErr = (A.flags & CVTTMI_FLAG_UNIFORM) != 0;

    best.err = FLT_MAX;
    best.ep0 = best.ep1 = 0;
    best.idxLo = best.idxHi = 0;
    const int myCount = active ? count : 0; // member i exists for i < myCount
    const u32 listLo = (u32)list, listHi = (u32)(list >> 32);
    // pixel id of member i (i is wave-uniform: the halves of the list are told apart by a scalar branch)
    auto memberOf = [&](int i) -> int {
        return (int)(i < 8 ? __builtin_amdgcn_ubfe(listLo, (u32)(4 * i), 4u) : __builtin_amdgcn_ubfe(listHi, (u32)(4 * i - 32), 4u));
    };
#ifdef CVTT_BC7_PROFILE
    u32 profHist[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
#endif

    // static alpha error of RGB modes (reference BC67.cpp:1250-1264); zero on opaque blocks
    float staticAlphaError = 0.0f;
    if (isRGB)
    {
        u32 acc = 0;
        for (int i = 0; i < maxCount; i++)
        {
            if (i < myCount)
            {
                const int d = 255 - byteI(lp[memberOf(i)], 3);
                acc = (u32)mad24(d, d, (int)acc);
            }
        }
        staticAlphaError = uniformErr ? (float)(int)acc : (float)(int)acc * A.wSq[3];
    }

    // UnfinishedEndpoints::FinishLDR (reference UnfinishedEndpoints.h:77-91)
    const float tf0 = T->tweakFactors[md.indexBits - 2][tweak][0];
    const float tf1 = T->tweakFactors[md.indexBits - 2][tweak][1];
    int ep[2][4];
    const int firstRound = split ? split->firstRound : 0, endRound = split ? split->endRound : numRefine;
    if (firstRound > 0)
    {
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
        {
            ep[0][ch] = byteI(split->ep0, ch);
            ep[1][ch] = byteI(split->ep1, ch);
        }
    }
    else
    {
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
        {
            if (ch < NRC)
            {
                ep[0][ch] = endpointByte(u.base[ch] + u.offset[ch] * tf0);
                ep[1][ch] = endpointByte(u.base[ch] + u.offset[ch] * tf1);
            }
            else
                ep[0][ch] = ep[1][ch] = 255;
        }
    }

    for (int refine = firstRound; refine < endRound; refine++)
    {
        const bool last = (refine == numRefine - 1);
        if (refine > firstRound || firstRound == 0)
            compressEndpoints(md, ep, pIter, isRGB);
        if (split && refine == firstRound)
        {
            split->r0ep0 = packEP(ep[0]);
            split->r0ep1 = packEP(ep[1]);
        }
#ifdef CVTT_BC7_PROFILE
        {
            const u32 k0 = packEP(ep[0]), k1 = packEP(ep[1]);
            const int ln = (int)threadIdx.x;
            bool dupNow = false, dupOld = false;
            for (int o = 0; o < 4; o++)
            {
                const int src = (ln & ~3) | o;
                const u32 a0 = __shfl(k0, src), a1 = __shfl(k1, src);
                const bool oAct = __shfl((int)active, src) != 0;
                if (oAct && o < (ln & 3) && a0 == k0 && a1 == k1) dupNow = true;
                for (int h = 0; h < refine && h < 4; h++)
                {
                    const u32 b0 = __shfl(profHist[h][0], src), b1 = __shfl(profHist[h][1], src);
                    if (oAct && b0 == k0 && b1 == k1) dupOld = true;
                }
            }
            if (refine < 4) { profHist[refine][0] = k0; profHist[refine][1] = k1; }
            const u64 mA = __ballot(active), mN = __ballot(active && dupNow), mO = __ballot(active && !dupNow && dupOld);
            if (ln == 0)
            {
                atomicAdd(&g_bc7Dup[0], (unsigned long long)__popcll(mA));
                atomicAdd(&g_bc7Dup[1], (unsigned long long)__popcll(mN));
                atomicAdd(&g_bc7Dup[2], (unsigned long long)__popcll(mO));
                atomicAdd(&g_bc7Dup[3 + (refine < 3 ? refine : 3)], (unsigned long long)__popcll(mN | mO));
            }
        }
#endif

        // IndexSelector<4>::Init (reference IndexSelector.h:27-77)
        float origin[4], axis[4];
        int recBase[4], recDelta[4];
        {
            float epDW[4];
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
            {
                origin[ch] = (float)ep[0][ch];
                epDW[ch] = ((float)ep[1][ch] - origin[ch]) * A.w[ch];
                // scaled by 4: the reconstructed value (x >> 6) is then byte 1 of the sum
                recBase[ch] = ((ep[0][ch] << 6) + 32) << 2;
                recDelta[ch] = (ep[1][ch] - ep[0][ch]) << 2;
            }
            float lenSq = epDW[0] * epDW[0];
#pragma unroll
            for (int ch = 1; ch < 4; ch++)
                lenSq = lenSq + epDW[ch] * epDW[ch];
            lenSq = safeDenom(lenSq);
            const float mvdls = maxValue / lenSq;
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
                axis[ch] = epDW[ch] * A.w[ch] * mvdls;
        }

        const v2f org01 = {origin[0], origin[1]}, org23 = {origin[2], origin[3]};
        const v2f ax01 = {axis[0], axis[1]}, ax23 = {axis[2], axis[3]};
        const v2f w01 = {A.w[0], A.w[1]}, w23 = {A.w[2], A.w[3]};
        u32 err[4] = {0, 0, 0, 0};
        float slowErr = 0.0f;
        v2f tv01 = {0.0f, 0.0f}, tv23 = {0.0f, 0.0f};
        float tt = 0.0f, ts = 0.0f;
        u32 idxLo = 0, idxHi = 0; // compact: member i in bits [4i, 4i + 4)

        for (int i = 0; i < maxCount; i++)
        {
            if (i < myCount)
            {
                const u32 pk = lp[memberOf(i)];
                // SelectIndexLDR (reference IndexSelector.h:124-131)
                const v2f x01 = {byteF(pk, 0), byteF(pk, 1)}, x23 = {byteF(pk, 2), byteF(pk, 3)};
                const v2f p01 = (x01 - org01) * ax01, p23 = (x23 - org23) * ax23;
                float dist = p01.x + p01.y;
                dist = dist + p23.x;
                dist = dist + p23.y;
                float fidx = clampRound(dist, maxValue);
                int index = (int)fidx;

                if (FAST)
                {
                    // ReconstructLDR_BC7 + ComputeErrorLDR (IndexSelector.h:90-100, BCCommon.h:24-29)
                    const int wgt = mad24(weightRcp, index, 256) >> 9;
                    err[0] = accumulateChannelError<0>(wgt, recDelta[0], recBase[0], pk, err[0]);
                    err[1] = accumulateChannelError<1>(wgt, recDelta[1], recBase[1], pk, err[1]);
                    err[2] = accumulateChannelError<2>(wgt, recDelta[2], recBase[2], pk, err[2]);
                    if (NRC == 4)
                        err[3] = accumulateChannelError<3>(wgt, recDelta[3], recBase[3], pk, err[3]);
                }
                else
                {
                    // slow indexing: also probe index-1 / index+1 (reference BC67.cpp:1367-1386)
                    float bestE = 0.0f;
                    const int index0 = index;
#pragma unroll
                    for (int probe = 0; probe < 3; probe++)
                    {
                        int cand = index0;
                        if (probe == 1) cand = (index0 > 1 ? index0 : 1) - 1;
                        if (probe == 2) cand = (index0 + 1 < range - 1) ? index0 + 1 : range - 1;
                        const int wgt = mad24(weightRcp, cand, 256) >> 9;
                        // the reconstructed channel is byte 1 of w * delta4 + base4; its difference to the pixel and the
                        // square are taken as floats (exact on these integers, see evalDual: plain f32 instructions)
                        const float xs[4] = {x01.x, x01.y, x23.x, x23.y};
                        float e4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int ch = 0; ch < NRC; ch++)
                        {
                            const float d = byteF((u32)madI24(wgt, recDelta[ch], recBase[ch]), 1) - xs[ch];
                            e4[ch] = d * d;
                        }
                        float e;
                        if (uniformErr)
                            e = ((e4[0] + e4[1]) + e4[2]) + e4[3];
                        else
                        {
                            e = e4[0] * A.wSq[0];
                            e = e + e4[1] * A.wSq[1];
                            e = e + e4[2] * A.wSq[2];
                            e = e + e4[3] * A.wSq[3];
                        }
                        if (probe == 0)
                            bestE = e;
                        else
                        {
                            // both alternatives derive from the initial index (BC67.cpp:1367-1386); the winner is tracked as an
                            // integer and converted once, and the comparison that moves it also serves the minimum
                            const bool better = e < bestE;
                            bestE = better ? e : bestE;
                            index = better ? cand : index;
                        }
                    }
                    slowErr = slowErr + bestE;
                    fidx = (float)index;
                }

                if (!last)
                {
                    // EndpointRefiner::ContributeUnweightedPW (EndpointRefiner.h:78-92)
                    const float t = fidx * rcpMaxIndex;
                    const v2f t2 = {t, t};
                    const v2f v01 = x01 * w01, v23 = x23 * w23; // channel 3 is unused when NRC == 3
                    tv01 = tv01 + t2 * v01;
                    tv23 = tv23 + t2 * v23;
                    tt = tt + t * t;
                    ts = ts + t;
                }
                if (wantPayload)
                {
                    if (i < 8)
                        idxLo |= (u32)index << (4 * i);
                    else
                        idxHi |= (u32)index << (4 * i - 32);
                }
            }
        }

        // AggregatedError<4>::Finalize (reference AggregatedError.h:29-46)
        float shapeError;
        if (FAST)
        {
            if (uniformErr)
                shapeError = (float)(int)(err[0] + err[1] + err[2] + err[3]);
            else
            {
                shapeError = (float)(int)err[0] * A.wSq[0];
                shapeError = shapeError + (float)(int)err[1] * A.wSq[1];
                shapeError = shapeError + (float)(int)err[2] * A.wSq[2];
                shapeError = shapeError + (float)(int)err[3] * A.wSq[3];
            }
        }
        else
            shapeError = slowErr;
        if (isRGB)
            shapeError = shapeError + staticAlphaError;

        if (TRACE && active)
        {
            // (two pointers, not one: the LDS stores stay ds_write instead of turning into flat stores)
            if (trialErrHbm)
                trialErrHbm[refine] = shapeError;
            else if (trialErr)
                trialErr[refine] = shapeError;
        }
        const bool take = (TRACE && captureRound >= 0) ? (refine == captureRound) : (shapeError < best.err);
        if (active && take)
        {
            best.err = shapeError;
            best.ep0 = packEP(ep[0]);
            best.ep1 = packEP(ep[1]);
            best.idxLo = idxLo;
            best.idxHi = idxHi;
        }

        if (!last)
        {
            // EndpointRefiner::GetRefinedEndpointsLDR (EndpointRefiner.h:99-152)
            const float tv[4] = {tv01.x, tv01.y, tv23.x, tv23.y};
            float adenom = (tt * wCount - ts * ts) * wRcp;
            const bool adenomZero = (adenom == 0.0f);
            if (adenomZero)
                adenom = 1.0f;
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
            {
                if (ch < NRC)
                {
                    const float a = (tv[ch] - ts * vs[ch] * wRcp) / adenom;
                    const float b = (vs[ch] - a * ts) * wRcp;
                    float p1 = b;
                    float p2 = a + b;
                    if (adenomZero)
                    {
                        p1 = vs[ch] * wRcp;
                        p2 = p1;
                    }
                    ep[0][ch] = endpointByte(p1 * A.rcpW[ch]);
                    ep[1][ch] = endpointByte(p2 * A.rcpW[ch]);
                }
                else
                    ep[0][ch] = ep[1][ch] = 0; // overwritten with 255 by compressEndpoints
            }
        }
    }
    if (split && endRound < numRefine)
    {
        compressEndpoints(md, ep, pIter, isRGB);
        split->ep0 = packEP(ep[0]);
        split->ep1 = packEP(ep[1]);
    }
}

// Order-preserving argmin over aligned groups of `width` lanes (4, 8 or 16): ties go to the
// lower lane, i.e. the earlier chain in the reference's sequential commit order.
__device__ __forceinline__ void groupArgminBroadcast(ShapeBest &b, int lane, int width)
{
    int who = lane;
    float err = b.err;
    // (width is 4, 8 or 16, wave-uniform: the steps are spelled out so that each is a ds_swizzle with a literal pattern)
#define CVTT_GROUP_STEP(STEP)                                             \
    {                                                                     \
        const float oErr = xorLane(err, STEP);                            \
        const int oWho = xorLane(who, STEP);                              \
        const bool take = (oErr < err) || (oErr == err && oWho < who);    \
        err = take ? oErr : err;                                          \
        who = take ? oWho : who;                                          \
    }
    CVTT_GROUP_STEP(1)
    CVTT_GROUP_STEP(2)
    if (width > 4)
        CVTT_GROUP_STEP(4)
    if (width > 8)
        CVTT_GROUP_STEP(8)
#undef CVTT_GROUP_STEP
    b.err = err;
    b.ep0 = __shfl(b.ep0, who);
    b.ep1 = __shfl(b.ep1, who);
    b.idxLo = __shfl(b.idxLo, who);
    b.idxHi = __shfl(b.idxHi, who);
}

// Pixel source for the PCA passes of a block staged in LDS.
struct FetchLDS
{
    const u32 *lp;
    const float (&w)[4];
    template <int N>
    __device__ __forceinline__ void get(int px, float (&v)[N]) const
    {
        const u32 pk = lp[px];
#pragma unroll
        for (int ch = 0; ch < N; ch++)
            v[ch] = byteF(pk, ch) * w[ch];
    }
};

template <int N>
__device__ __forceinline__ void pcaEndpointsLDS(const u32 *lp, u32 mask, const float (&w)[4], Unfinished &u, float *sums)
{
    const FetchLDS F = {lp, w};
    Moments<N> m;
    pcaMomentsT<N>(F, mask, m, sums);
    pcaFinishT<N>(F, mask, w, m, u);
}

// What one lane of the PCA pass leaves for the chain lanes of its (block, partition, subset).
struct UnitRec
{
    float base[4];
    float offset[4];
    u32 packed;  // mask | numTweak << 16 | blk << 20 | slot << 24  (slot = item * subsets + subset: where the subset's result goes)
    float scErr; // BC7_TrySingleColor: error of the fixed candidate (FLT_MAX when not tried)
    // the refiner's m_v of the subset: sum of the pre-weighted member pixels in ascending order (EndpointRefiner.h:78-92).
    // It does not depend on the indexes, so the seed lane takes it once for all chains and rounds of the unit.
    float vs[4];
    // the member pixels of the subset in ascending order, 4 bits each: the chain lanes read pixel i of their subset with one
    // bit-field extract at a wave-uniform position instead of popping a per-lane bit mask
    u32 listLo, listHi;
    __device__ __forceinline__ u32 mask() const { return packed & 0xffffu; }
    __device__ __forceinline__ int numTweak() const { return (int)((packed >> 16) & 7u); }
    __device__ __forceinline__ int blk() const { return (int)((packed >> 20) & 15u); }
    __device__ __forceinline__ int slot() const { return (int)(packed >> 24); }
};

struct WorkState
{
    float err;
    int mode;
    int partOrIS; // partition, or index selector for modes 4/5 (union in the reference, BC67.cpp:67-75)
    int rotation;
    u32 ep[3][2];
    u32 idxLo, idxHi;   // primary indexes, 4 bits per pixel (modes 4/5: in the slots of dualIndexSlot, else by pixel position)
    u32 idx2Lo, idx2Hi; // secondary indexes (modes 4/5, in the slots of dualIndexSlot)
};

// Fix-ups + bit packing of a mode 4 / mode 5 block (reference BC67.cpp:2003-2203) by one lane: with the mode a template
// parameter every field sits at a constant bit position, so the 66 fields cost a shift-or each instead of the generic
// packer's per-lane field arithmetic (the kernel keeps that one for the other modes).
template <int MODE>
__device__ __forceinline__ void packDualPlane(const WorkState &work, u32 &w0, u32 &w1, u32 &w2, u32 &w3)
{
    constexpr int rgbBits = (MODE == 4) ? 5 : 7, alphaBits = (MODE == 4) ? 6 : 8, alphaIndexBits = (MODE == 4) ? 3 : 2;
    constexpr u32 idxOnes = 0x33333333u, idx2Ones = (MODE == 4) ? 0x77777777u : 0x33333333u;
    u32 iLo = work.idxLo, iHi = work.idxHi, jLo = work.idx2Lo, jHi = work.idx2Hi;
    // the anchor (pixel 0) of either index set must have its top bit clear: complement the set and exchange the
    // endpoints it interpolates (every 4-bit slot holds at most the set's maximum, so the complement is an XOR)
    bool flipRGB = ((iLo >> 1) & 1u) != 0;
    bool flipAlpha = ((jLo >> (alphaIndexBits - 1)) & 1u) != 0;
    if (flipRGB)
    {
        iLo ^= idxOnes;
        iHi ^= idxOnes;
    }
    if (flipAlpha)
    {
        jLo ^= idx2Ones;
        jHi ^= idx2Ones;
    }
    const int indexSelector = (MODE == 4) ? work.partOrIS : 0;
    if (indexSelector)
    {
        const bool t = flipRGB;
        flipRGB = flipAlpha;
        flipAlpha = t;
    }
    u32 e0 = work.ep[0][0], e1 = work.ep[0][1];
    if (flipRGB)
    {
        const u32 a = e0, b = e1;
        e0 = (a & 0xff000000u) | (b & 0x00ffffffu);
        e1 = (b & 0xff000000u) | (a & 0x00ffffffu);
    }
    if (flipAlpha)
    {
        const u32 a = e0, b = e1;
        e0 = (a & 0x00ffffffu) | (b & 0xff000000u);
        e1 = (b & 0x00ffffffu) | (a & 0xff000000u);
    }
    u64 lo = 0, hi = 0;
    auto put = [&](u32 value, int off) {
        const u64 v = (u64)value;
        if (off < 64)
        {
            lo |= v << off;
            if (off > 56)
                hi |= v >> (64 - off); // fields are at most 8 bits wide
        }
        else
            hi |= v << (off - 64);
    };
    put(1u << MODE, 0);
    put((u32)work.rotation, MODE + 1);
    if (MODE == 4)
        put((u32)indexSelector, 7);
    constexpr int epBase = 8;
#pragma unroll
    for (int g = 0; g < 6; g++)
    {
        const u32 e = (g & 1) ? e1 : e0;
        put(((e >> (8 * (g >> 1))) & 0xffu) >> (8 - rgbBits), epBase + g * rgbBits);
    }
    constexpr int alphaBase = epBase + 6 * rgbBits;
    put((e0 >> 24) >> (8 - alphaBits), alphaBase);
    put((e1 >> 24) >> (8 - alphaBits), alphaBase + alphaBits);
    constexpr int idxBase = alphaBase + 2 * alphaBits;
    // (the index sets arrive in the search's layout: pixel px in slot dualIndexSlot(px), a constant shift like any other)
#pragma unroll
    for (int px = 0; px < 16; px++)
        put(((px < 8 ? iLo : iHi) >> (4 * dualIndexSlot(px))) & 0xfu, idxBase + 2 * px - (px > 0 ? 1 : 0));
    constexpr int idx2Base = idxBase + 31;
#pragma unroll
    for (int px = 0; px < 16; px++)
        put(((px < 8 ? jLo : jHi) >> (4 * dualIndexSlot(px))) & 0xfu, idx2Base + alphaIndexBits * px - (px > 0 ? 1 : 0));
    w0 = (u32)lo;
    w1 = (u32)(lo >> 32);
    w2 = (u32)hi;
    w3 = (u32)(hi >> 32);
}

} // namespace
