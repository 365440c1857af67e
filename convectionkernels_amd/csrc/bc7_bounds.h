// BC7 partition bounds.  Part of bc7_kernel.hip (one translation unit), included after bc7_dual.h.
#pragma once

namespace
{
// =====================================================================================
// Exact branch-and-bound, part 2: cheap bounds for every partition before anything is
// searched (part 1, the bound itself, is shapeErrorLowerBound in cvtt_kernel_common.h).
//
// The weighted pixels of a block are projected on an orthonormal pair (e1, e2) -- the two
// leading principal axes of the whole block, so that little of any subset's residual is lost --
// scaled and rounded to 12-bit integers.  An orthogonal projection never increases distances,
// so the total-least-squares residual of the projected, rounded points (minus the allowance
// for the rounding radius) still bounds the error of every trial from below; in 2-D the
// residual is the smaller eigenvalue of a 2x2 matrix whose entries are exact integers
// accumulated with v_dot2_i32_i16 over a per-lane pixel mask.  Sub-lane c of a quad walks
// partitions c, c+4, ...; the bounds land in LDS (64 partitions x 16 blocks).
// =====================================================================================
typedef short v2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(u32 a, u32 b, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, a), __builtin_bit_cast(v2s, b), acc, false);
}

__device__ __forceinline__ constexpr int tri(int r, int c) { return r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r; }

struct BlockScatter
{
    float S[10];     // weighted scatter matrix of the 16 pixels (lower triangle, row-major)
    float meanW[4];  // weighted centroid
};

// raw sums of the 16 pixels: s[ch] = sum x, p[tri(r, c)] = sum x_r x_c, by the four lanes of the quad that holds the block:
// sub-lane c sums pixels c, c+4, c+8, c+12 and the quad adds up
__device__ __forceinline__ void blockRawSumsQuad(const u32 (&pix)[16], int c, int (&s)[4], int (&p)[10])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
        s[i] = 0;
#pragma unroll
    for (int i = 0; i < 10; i++)
        p[i] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
        const u32 p0 = pix[4 * j], p1 = pix[4 * j + 1], p2 = pix[4 * j + 2], p3 = pix[4 * j + 3];
        const u32 pk = fetchPixel(c == 0 ? p0 : c == 1 ? p1 : c == 2 ? p2 : p3);
        int x[4];
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
        {
            x[ch] = byteI(pk, ch);
            s[ch] += x[ch];
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int cc = 0; cc <= r; cc++)
                p[tri(r, cc)] = mad24(x[r], x[cc], p[tri(r, cc)]);
    }
#pragma unroll
    for (int step = 1; step <= 2; step <<= 1)
    {
#pragma unroll
        for (int i = 0; i < 4; i++)
            s[i] += xorLane(s[i], step);
#pragma unroll
        for (int i = 0; i < 10; i++)
            p[i] += xorLane(p[i], step);
    }
}

__device__ __forceinline__ void scatterFromRaw(const int (&s)[4], const int (&p)[10], const CvttBc7Args &A, BlockScatter &bs)
{
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        bs.meanW[r] = (float)s[r] * A.w[r] * 0.0625f;
#pragma unroll
        for (int c = 0; c <= r; c++)
        {
            // 16*sum(xy) - sum(x)*sum(y): an exact integer below 2^24
            const int v = 16 * p[tri(r, c)] - __mul24(s[r], s[c]);
            // (no product of two weights on its own: the optimiser would keep all ten of them in registers for the whole kernel)
            bs.S[tri(r, c)] = (((float)v * 0.0625f) * A.w[r]) * A.w[c];
        }
    }
}

// Exact branch-and-bound, second tier: the bound of a subset in all of its channels.  The 2-D projection of the first
// tier keeps one of the three (two) residual directions of a subset; on low-variance content with noise in every
// channel that leaves most partitions alive.  Raw integer sums of the member pixels of a subset -> scatter matrix ->
// shapeErrorLowerBound, for the partitions that survived the first tier only.
struct RawSums
{
    int n;
    int s[4];
    int p[10];
};

// channel-major copy of a block: P[ch][g] = channel ch of pixels 4g .. 4g+3 (the layout of the dual-plane search)
__device__ __forceinline__ void channelMajor(const u32 (&pix)[16], u32 (&P)[4][4])
{
#pragma unroll
    for (int g = 0; g < 4; g++)
    {
        const u32 a = fetchPixel(pix[4 * g]), b = fetchPixel(pix[4 * g + 1]), cc = fetchPixel(pix[4 * g + 2]), d = fetchPixel(pix[4 * g + 3]);
        const u32 ab02 = __builtin_amdgcn_perm(b, a, 0x06020400u); // a0 b0 a2 b2
        const u32 ab13 = __builtin_amdgcn_perm(b, a, 0x07030501u); // a1 b1 a3 b3
        const u32 cd02 = __builtin_amdgcn_perm(d, cc, 0x06020400u);
        const u32 cd13 = __builtin_amdgcn_perm(d, cc, 0x07030501u);
        P[0][g] = __builtin_amdgcn_perm(cd02, ab02, 0x05040100u); // a0 b0 c0 d0
        P[2][g] = __builtin_amdgcn_perm(cd02, ab02, 0x07060302u); // a2 b2 c2 d2
        P[1][g] = __builtin_amdgcn_perm(cd13, ab13, 0x05040100u);
        P[3][g] = __builtin_amdgcn_perm(cd13, ab13, 0x07060302u);
    }
}

// the sums of the member pixels of `mask` (a pixel that is not a member counts as (0, 0, 0, 0)) from the channel-major copy:
// four pixels per v_dot4_u32_u8
__device__ __forceinline__ void maskedRawSumsCM(const u32 (&P)[4][4], u32 mask, RawSums &r)
{
    r.n = __popc(mask & 0xffffu);
#pragma unroll
    for (int i = 0; i < 4; i++)
        r.s[i] = 0;
#pragma unroll
    for (int i = 0; i < 10; i++)
        r.p[i] = 0;
#pragma unroll
    for (int g = 0; g < 4; g++)
    {
        // four mask bits -> four 0x00 / 0xff bytes
        const u32 bits = (((mask >> (4 * g)) & 0xfu) * 0x00204081u) & 0x01010101u;
        const u32 sel = (bits << 8) - bits;
        u32 m[4];
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
        {
            m[ch] = P[ch][g] & sel;
            r.s[ch] = (int)__builtin_amdgcn_udot4(m[ch], 0x01010101u, (u32)r.s[ch], false);
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b <= a; b++)
                r.p[tri(a, b)] = (int)__builtin_amdgcn_udot4(m[a], P[b][g], (u32)r.p[tri(a, b)], false);
    }
}

__device__ __forceinline__ void rawSumsSub(RawSums &d, const RawSums &a)
{
    d.n -= a.n;
#pragma unroll
    for (int i = 0; i < 4; i++)
        d.s[i] -= a.s[i];
#pragma unroll
    for (int i = 0; i < 10; i++)
        d.p[i] -= a.p[i];
}

// n*sum(xy) - sum(x)*sum(y) is an exact integer below 2^24, so the matrix entries carry the rounding of two float
// products only, which the margins of shapeErrorLowerBound cover
template <int N>
__device__ __forceinline__ float subsetBoundFull(const RawSums &r, const float (&w)[4], float delta)
{
    if (r.n < 2)
        return 0.0f;
    const float n = (float)r.n;
    const float inv = __builtin_amdgcn_rcpf(n);
    Moments<N> m;
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
        for (int b = 0; b <= a; b++)
        {
            const int v = __mul24(r.n, r.p[tri(a, b)]) - __mul24(r.s[a], r.s[b]);
            m.cov[tri(a, b)] = (((float)v * inv) * w[a]) * w[b]; // see scatterFromRaw
        }
    return shapeErrorLowerBound<N>(m, n, delta);
}

// dominant eigenvector of a symmetric PSD 4x4 (power iteration from the column of the
// largest diagonal entry).  Accuracy only affects how tight the bounds are, never their
// validity: the caller orthonormalises whatever comes back.
__device__ __forceinline__ void topEigenvector(const float (&M)[10], float (&e)[4])
{
    int k = 0;
    float d = M[tri(0, 0)];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (M[tri(i, i)] > d)
        {
            d = M[tri(i, i)];
            k = i;
        }
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        v[i] = (k == 0) ? M[tri(i, 0)] : (k == 1) ? M[tri(i, 1)] : (k == 2) ? M[tri(i, 2)] : M[tri(i, 3)];
    for (int it = 0; it < CVTT_EIG_ITERS; it++)
    {
        float nv[4];
        float big = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            float a = M[tri(r, 0)] * v[0];
#pragma unroll
            for (int c = 1; c < 4; c++)
                a = __fmaf_rn(M[tri(r, c)], v[c], a);
            nv[r] = a;
            big = fmaxf(big, fabsf(a));
        }
        const float sc = (big > 0.0f) ? __builtin_amdgcn_rcpf(big) : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++)
            v[r] = nv[r] * sc;
    }
    float len = v[0] * v[0];
#pragma unroll
    for (int i = 1; i < 4; i++)
        len = __fmaf_rn(v[i], v[i], len);
    const bool ok = len > 1e-12f && len < 1e12f; // false for 0 and NaN
    const float inv = ok ? __builtin_amdgcn_rsqf(len) : 0.0f;
    e[0] = ok ? v[0] * inv : 1.0f;
#pragma unroll
    for (int i = 1; i < 4; i++)
        e[i] = v[i] * inv;
}

// Second tier, sharpened ("Soundness of the bounds", part 3).  The bound above treats a trial as ANY line plus
// the worst rounding of the reconstructed colours (delta = 0.5 * |w|, as if every rounding pointed at the pixel).  Two facts
// about the trials tighten it, both stated for an arbitrary unit vector d (here: the subset's principal direction from a few
// power iterations -- its accuracy affects only how tight the result is):
//  * Rounding moves a reconstructed colour by at most 0.5 * w_ch per channel, and only the part of that ACROSS the trial's
//    line lowers the error.  For a line along u the largest such part is s(u) = 0.5 * sqrt(|w|^2 - min_sigma (u . (sigma w))^2)
//    (sigma = sign patterns).  With the default channel weights (green and alpha dominate) and a line that follows green, s is
//    0.16 instead of 0.52.
//  * The reconstructed colours of a subset are only 2^indexBits points of the line.  Projected on d the pixels are therefore
//    approximated by that many values: Q_d = the cost of the best clustering of the projections into 2^indexBits groups
//    (sum of squared distances to the group means).  It is computed for the two-bit modes, exactly: the projections are
//    sorted (the groups of an optimal clustering in one dimension are runs) and a dynamic programme places the boundaries.
// A trial whose line u makes the angle asin(beta) with d (u = alpha d + beta v, v _|_ d) has, before rounding,
//    error >= alpha^2 R_d + beta^2 L_d - 2 alpha beta rho + max(0, alpha sqrt(Q_d) - beta sqrt(R_d))^2,
// L_d = d^T S d, R_d = trace(S) - L_d (>= v^T S v), rho = |S d - L_d d| (>= |d^T S v|); the last term is the distance of the
// projections on u from the (cone of) vectors with few distinct values, which differs from that of the projections on d by at
// most beta sqrt(v^T S v).  And |u . (sigma w)| >= alpha m_d - beta sqrt(|w|^2 - m_d^2) with m_d = min_sigma |d . (sigma w)|
// (>= 2 max_ch - sum_ch of |d_ch| w_ch).  [0, 1] is cut into a few intervals of beta; on each, every term is replaced by its worst
// value there, G - 2 s sqrt(n G) is formed as in the first bound, and the minimum over the intervals is the result.  Margins:
// every quantity that comes from a cancellation is moved by 1e-5 * trace(S) in the safe direction (the float error of S, of d's
// length and of the products is below 2e-6 of it), the projections by 2e-3, the result is scaled by 0.9999.
// (lp: the block's sixteen pixels in LDS.  They are read twice, for the sums and for the projections, rather than kept in
// registers in between: this function is the register peak of the bounds.)
template <int N>
__device__ __forceinline__ float subsetBoundSharp(const u32 *lp, u32 mask, const float (&w)[4], float delta, float wSq, bool fourLevels
#ifdef CVTT_BC7_BOUND_DUMP
                                                  , float (&dUsed)[4] // the bound dump: the direction d (zeros when the plain bound is all there is)
#endif
)
{
#ifdef CVTT_BC7_BOUND_DUMP
    dUsed[0] = dUsed[1] = dUsed[2] = dUsed[3] = 0.0f;
#endif
    RawSums r;
    {
        asm volatile("" : "+v"(lp));
        u32 px[16], CM[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const uint4 v = *reinterpret_cast<const uint4 *>(lp + 4 * i);
            px[4 * i + 0] = v.x;
            px[4 * i + 1] = v.y;
            px[4 * i + 2] = v.z;
            px[4 * i + 3] = v.w;
        }
        channelMajor(px, CM);
        maskedRawSumsCM(CM, mask, r);
    }
    if (r.n < 2)
        return 0.0f;
    const float n = (float)r.n;
    const float inv = __builtin_amdgcn_rcpf(n);
    Moments<N> m;
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
        for (int b = 0; b <= a; b++)
        {
            const int v = __mul24(r.n, r.p[tri(a, b)]) - __mul24(r.s[a], r.s[b]);
            m.cov[tri(a, b)] = (((float)v * inv) * w[a]) * w[b]; // see scatterFromRaw
        }
    float rTrue;
    const float cur = shapeErrorLowerBound<N>(m, n, delta, &rTrue);
    if (r.n < 3 || !(rTrue >= 0.0f))
        return cur;
    float T = 0.0f;
#pragma unroll
    for (int i = 0; i < N; i++)
        T += m.cov[tri(i, i)];
    float e[4];
    {
        float M[10];
#pragma unroll
        for (int i = 0; i < 10; i++)
            M[i] = (N == 4 || i < 6) ? m.cov[i < N * (N + 1) / 2 ? i : 0] : 0.0f;
        topEigenvector(M, e);
    }
#ifdef CVTT_BC7_BOUND_DUMP
#pragma unroll
    for (int i = 0; i < 4; i++)
        dUsed[i] = (i < N) ? e[i] : 0.0f;
#endif
    float L = 0.0f, Sd[N];
#pragma unroll
    for (int a = 0; a < N; a++)
    {
        float acc = 0.0f;
#pragma unroll
        for (int b = 0; b < N; b++)
            acc = __fmaf_rn(m.cov[a >= b ? tri(a, b) : tri(b, a)], e[b], acc);
        Sd[a] = acc;
        L = __fmaf_rn(e[a], acc, L);
    }
    float rho2 = 0.0f, aMax = 0.0f, aSum = 0.0f;
#pragma unroll
    for (int a = 0; a < N; a++)
    {
        const float t = Sd[a] - L * e[a];
        rho2 = __fmaf_rn(t, t, rho2);
        const float ac = fabsf(e[a]) * w[a];
        aMax = fmaxf(aMax, ac);
        aSum += ac;
    }
    const float eta = 1e-5f * T;
    const float Llo = fmaxf(L - eta, 0.0f);
    const float Rlo = fmaxf(T - L - eta, 0.0f);
    const float sqrtRhi = __builtin_amdgcn_sqrtf(fmaxf(T - L, 0.0f) + eta) * 1.000001f;
    const float rhoHi = __builtin_amdgcn_sqrtf(rho2) * 1.000001f + eta;
    const float W2 = wSq * 1.000001f;
    const float md = fmaxf(2.0f * aMax - aSum, 0.0f) * 0.99999f;
    const float perp = __builtin_amdgcn_sqrtf(fmaxf(W2 - md * md, 0.0f)) * 1.000001f;

    float sqrtQ = 0.0f;
    constexpr int kMaxN = 13; // the largest subset of any BC7 partition (a larger one would simply go without Q_d)
    if (fourLevels && r.n > 4 && r.n <= kMaxN)
    {
        float g[4];
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
            g[ch] = (ch < N) ? e[ch] * w[ch] : 0.0f;
        float t[16];
        asm volatile("" : "+v"(lp));
#pragma unroll
        for (int q = 0; q < 4; q++)
        {
            const uint4 v = *reinterpret_cast<const uint4 *>(lp + 4 * q);
            const u32 pw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                float a = 0.0f;
#pragma unroll
                for (int ch = 0; ch < N; ch++)
                    a = __fmaf_rn(g[ch], byteF(pw[k], ch), a);
                t[4 * q + k] = ((mask >> (4 * q + k)) & 1u) ? a : 1e30f;
            }
        }
        // Batcher's merge exchange, 63 comparators: the members come first, in ascending order
#define CE(a, b) { const float lo_ = fminf(t[a], t[b]); t[b] = fmaxf(t[a], t[b]); t[a] = lo_; }
        CE(0,1) CE(2,3) CE(4,5) CE(6,7) CE(8,9) CE(10,11) CE(12,13) CE(14,15) CE(0,2) CE(1,3) CE(4,6) CE(5,7) CE(8,10) CE(9,11) CE(12,14) CE(13,15)
        CE(1,2) CE(5,6) CE(9,10) CE(13,14) CE(0,4) CE(1,5) CE(2,6) CE(3,7) CE(8,12) CE(9,13) CE(10,14) CE(11,15) CE(2,4) CE(3,5) CE(10,12) CE(11,13)
        CE(1,2) CE(3,4) CE(5,6) CE(9,10) CE(11,12) CE(13,14) CE(0,8) CE(1,9) CE(2,10) CE(3,11) CE(4,12) CE(5,13) CE(6,14) CE(7,15) CE(4,8) CE(5,9)
        CE(6,10) CE(7,11) CE(2,4) CE(3,5) CE(6,8) CE(7,9) CE(10,12) CE(11,13) CE(1,2) CE(3,4) CE(5,6) CE(7,8) CE(9,10) CE(11,12) CE(13,14)
#undef CE
        // The exact cost of the best clustering of the sorted projections into four groups, by dynamic programming over the
        // group boundaries: D_k[j] = min_i D_(k-1)[i] + cost(i, j), cost(i, j) = sum t^2 - (sum t)^2 / (j - i) over t[i .. j-1]
        // (empty groups allowed: D_k[0] = 0).  Everything is unrolled over the kMaxN slots a subset can fill, the slots past the
        // members hold zeros after the shift by t[0], and the last group is taken from suffix sums so that no step depends on
        // the (per-lane) member count.
        const int cnt = r.n;
        const float t0 = t[0];
        float range = 0.0f;
#pragma unroll
        for (int j = 0; j < kMaxN; j++)
        {
            t[j] = (j < cnt) ? t[j] - t0 : 0.0f;
            range = fmaxf(range, t[j]);
        }
        constexpr float kRcp[17] = {0.0f, 1.0f, 1.0f / 2, 1.0f / 3, 1.0f / 4, 1.0f / 5, 1.0f / 6, 1.0f / 7, 1.0f / 8, 1.0f / 9, 1.0f / 10, 1.0f / 11, 1.0f / 12,
                                    1.0f / 13, 1.0f / 14, 1.0f / 15, 1.0f / 16};
        float D2[kMaxN + 1], D3[kMaxN + 1];
        D2[0] = D3[0] = 0.0f;
        {
            float su = 0.0f, sq = 0.0f;
#pragma unroll
            for (int j = 1; j <= kMaxN; j++)
            {
                su += t[j - 1];
                sq = __fmaf_rn(t[j - 1], t[j - 1], sq);
                D2[j] = D3[j] = __fmaf_rn(-su * su, kRcp[j], sq); // one group: D_1[j]
            }
        }
        float fin = D3[kMaxN]; // (zeros past the members: an over-estimate of the one-group cost of all of them, harmless in a minimum)
        {
            float su0 = 0.0f, sq0 = 0.0f; // prefix sums: D_1[i]
#pragma unroll
            for (int i = 1; i < kMaxN; i++)
            {
                su0 += t[i - 1];
                sq0 = __fmaf_rn(t[i - 1], t[i - 1], sq0);
                const float d1 = __fmaf_rn(-su0 * su0, kRcp[i], sq0);
                const float d2 = D2[i], d3 = D3[i]; // final: every start below i has been through
                float su = 0.0f, sq = 0.0f;
#pragma unroll
                for (int j = i + 1; j <= kMaxN; j++)
                {
                    su += t[j - 1];
                    sq = __fmaf_rn(t[j - 1], t[j - 1], sq);
                    const float cst = __fmaf_rn(-su * su, kRcp[j - i], sq);
                    D2[j] = fminf(D2[j], d1 + cst);
                    D3[j] = fminf(D3[j], d2 + cst);
                }
                // the fourth group, t[i .. cnt-1]: su / sq now hold the sums of everything from i on (zeros past the members)
                const float m = (float)(cnt - i);
                const float last = __fmaf_rn(-su * su, __builtin_amdgcn_rcpf(m), sq); // (v_rcp_f32: 1 ulp, inside the margin below)
                fin = (i < cnt) ? fminf(fin, d3 + last) : fin;
            }
        }
        // float error of a cost: a few ulps of (count * range^2); four of them and the running minima
        const float Q = fmaxf(fin - 2e-5f * range * range, 0.0f);
        sqrtQ = fmaxf(__builtin_amdgcn_sqrtf(fmaxf(Q * 0.9999f, 0.0f)) - 2e-3f, 0.0f);
    }

    // beta = 0, 0.01, 0.02, 0.03, 0.04, 0.055, 0.07, 0.085, 0.1, 0.125, 0.15, 0.175, 0.2, 0.25, 0.3, 0.375, 0.45, 0.55, 0.7, 0.85, 1: dense
    // where the minimum usually is (a small angle buys a lot of rounding slack when d is close to the dominant channel)
    constexpr int kIntervals = 20;
    constexpr float kB0sq[20] = {0.0f, 0.0001f, 0.0004f, 0.0009f, 0.0016f, 0.003025f, 0.0049f, 0.007225f, 0.01f, 0.015625f, 0.0225f, 0.030625f, 0.04f, 0.0625f, 0.09f, 0.140625f, 0.2025f, 0.3025f, 0.49f, 0.7225f};
    constexpr float kB1sq[20] = {0.0001f, 0.0004f, 0.0009f, 0.0016f, 0.003025f, 0.0049f, 0.007225f, 0.01f, 0.015625f, 0.0225f, 0.030625f, 0.04f, 0.0625f, 0.09f, 0.140625f, 0.2025f, 0.3025f, 0.49f, 0.7225f, 1.0f};
    constexpr float kB1[20] = {0.01f, 0.02f, 0.03f, 0.04f, 0.055f, 0.07f, 0.085f, 0.1f, 0.125f, 0.15f, 0.175f, 0.2f, 0.25f, 0.3f, 0.375f, 0.45f, 0.55f, 0.7f, 0.85f, 1.0f};
    // sqrt(1 - beta1^2), rounded down
    constexpr float kA1[20] = {0.999948f, 0.999798f, 0.9995479f, 0.9991977f, 0.9984844f, 0.997545f, 0.996379f, 0.9949854f, 0.9921548f, 0.988684f, 0.9845665f, 0.9797939f, 0.9682439f, 0.9539373f, 0.927023f, 0.8930268f, 0.835163f, 0.7141414f, 0.5267816f, 0.0f};
    // the largest alpha * beta of the interval, rounded up
    constexpr float kCross[20] = {0.00999952f, 0.01999604f, 0.02998656f, 0.03996807f, 0.05491686f, 0.06982843f, 0.08469255f, 0.09949894f, 0.1240198f, 0.1483032f, 0.1722998f, 0.1959596f, 0.2420619f, 0.2861823f, 0.347635f, 0.4018637f, 0.4593415f, 0.499901f, 0.500001f, 0.4477662f};
    float best = FLT_MAX;
#pragma unroll
    for (int j = 0; j < kIntervals; j++)
    {
        const float e0 = __fmaf_rn(kB0sq[j], Llo - Rlo, Rlo), e1 = __fmaf_rn(kB1sq[j], Llo - Rlo, Rlo);
        float base = fminf(e0, e1) * 0.999999f - 2.0f * kCross[j] * rhoHi;
        base = fmaxf(base, rTrue);
        const float qd = fmaxf(kA1[j] * sqrtQ - kB1[j] * sqrtRhi, 0.0f);
        const float G = __fmaf_rn(qd, qd, base);
        const float inner = fmaxf(kA1[j] * md - kB1[j] * perp, 0.0f);
        const float s2 = 0.25f * (W2 - inner * inner) * 1.000001f;
        float v = 0.0f;
        if (G > 4.0001f * n * s2)
            v = G - 2.0f * __builtin_amdgcn_sqrtf(s2 * n * G) * 1.000001f;
        best = fminf(best, v);
    }
    return fmaxf(cur, best * 0.9999f);
}

__device__ __forceinline__ int dot4s(u32 a, u32 b, int acc) { return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false); }
template <bool G8>
struct Proj2D
{
    // G8: int8 quadruples, pixel 4k + j in byte j; else int16 pairs, pixel 2k in the low half, 2k+1 in the high half
    u32 U[G8 ? 4 : 8], V[G8 ? 4 : 8];
    int tU, tV, tUU, tVV, tUV; // sums over all 16 pixels
};

// Project the block on its two leading principal axes (channels 0..2 only when !use4).
template <bool G8>
__device__ __forceinline__ void makeProjection(const u32 (&pix)[16], const BlockScatter &bs, const CvttBc7Args &A,
                                               bool use4, float scale, Proj2D<G8> &P)
{
    float M[10];
#pragma unroll
    for (int i = 0; i < 10; i++)
        M[i] = (use4 || i < 6) ? bs.S[i] : 0.0f;
    float e1[4], e2[4];
    topEigenvector(M, e1);
    {
        // deflate: M -= lambda e1 e1^T
        float Me[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            float a = M[tri(r, 0)] * e1[0];
#pragma unroll
            for (int c = 1; c < 4; c++)
                a = __fmaf_rn(M[tri(r, c)], e1[c], a);
            Me[r] = a;
        }
        float lam = Me[0] * e1[0];
#pragma unroll
        for (int r = 1; r < 4; r++)
            lam = __fmaf_rn(Me[r], e1[r], lam);
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c <= r; c++)
                M[tri(r, c)] = __fmaf_rn(-lam * e1[r], e1[c], M[tri(r, c)]);
    }
    topEigenvector(M, e2);
    {
        // Gram-Schmidt against e1; when nothing is left take the coordinate axis e1 leans on least
        float d = e2[0] * e1[0];
#pragma unroll
        for (int i = 1; i < 4; i++)
            d = __fmaf_rn(e2[i], e1[i], d);
        float len = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            e2[i] = __fmaf_rn(-d, e1[i], e2[i]);
            len = __fmaf_rn(e2[i], e2[i], len);
        }
        if (!(len > 1e-4f))
        {
            int k = 0;
            float small = fabsf(e1[0]);
#pragma unroll
            for (int i = 1; i < 4; i++)
                if ((use4 || i < 3) && fabsf(e1[i]) < small)
                {
                    small = fabsf(e1[i]);
                    k = i;
                }
            const float ek = (k == 0) ? e1[0] : (k == 1) ? e1[1] : (k == 2) ? e1[2] : e1[3];
            len = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                e2[i] = ((i == k) ? 1.0f : 0.0f) - ek * e1[i];
                len = __fmaf_rn(e2[i], e2[i], len);
            }
        }
        const float inv = __builtin_amdgcn_rsqf(len);
#pragma unroll
        for (int i = 0; i < 4; i++)
            e2[i] *= inv;
    }
    if (!use4)
        e1[3] = e2[3] = 0.0f; // already zero up to rounding; keep alpha out exactly

    float g1[4], g2[4];
    float o1 = 0.0f, o2 = 0.0f;
#pragma unroll
    for (int ch = 0; ch < 4; ch++)
    {
        g1[ch] = e1[ch] * A.w[ch] * scale;
        g2[ch] = e2[ch] * A.w[ch] * scale;
        o1 = __fmaf_rn(e1[ch] * scale, bs.meanW[ch], o1);
        o2 = __fmaf_rn(e2[ch] * scale, bs.meanW[ch], o2);
    }
    P.tU = P.tV = P.tUU = P.tVV = P.tUV = 0;
    if constexpr (G8)
    {
    // the four lanes of a quad hold the same block: sub-lane c projects pixels 4c .. 4c+3 and the quad exchanges the words
    int tid = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); // = threadIdx.x (one wave per workgroup), recomputed:
    asm volatile("" : "+v"(tid)); // the optimiser otherwise keeps the prologue's thread id (or `lane & ~3`) alive, spilled, for this
    const int c = tid & 3;
    u32 myU = 0, myV = 0;
    {
        u32 ub = 0, vb = 0;
#pragma unroll
        for (int h = 0; h < 4; h++)
        {
            const u32 p0 = pix[h], p1 = pix[4 + h], p2 = pix[8 + h], p3 = pix[12 + h];
            const u32 pk = fetchPixel(c == 0 ? p0 : c == 1 ? p1 : c == 2 ? p2 : p3);
            float fu = -o1, fv = -o2;
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
            {
                const float x = byteF(pk, ch);
                fu = __fmaf_rn(g1[ch], x, fu);
                fv = __fmaf_rn(g2[ch], x, fv);
            }
            // clamping is a projection on a box: it never increases distances either
            fu = fminf(fmaxf(fu, -kBoundLimit8), kBoundLimit8);
            fv = fminf(fmaxf(fv, -kBoundLimit8), kBoundLimit8);
            ub |= ((u32)(int)rintf(fu) & 0xffu) << (8 * h);
            vb |= ((u32)(int)rintf(fv) & 0xffu) << (8 * h);
        }
        myU = ub;
        myV = vb;
    }
    const int quadBase = tid & ~3;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const u32 ub = (u32)__shfl((int)myU, quadBase + k), vb = (u32)__shfl((int)myV, quadBase + k);
        P.U[k] = ub;
        P.V[k] = vb;
        P.tU = dot4s(ub, 0x01010101u, P.tU);
        P.tV = dot4s(vb, 0x01010101u, P.tV);
        P.tUU = dot4s(ub, ub, P.tUU);
        P.tVV = dot4s(vb, vb, P.tVV);
        P.tUV = dot4s(ub, vb, P.tUV);
    }
    }
    else
    {
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
        int uu[2], vv[2];
#pragma unroll
        for (int h = 0; h < 2; h++)
        {
            const u32 pk = fetchPixel(pix[2 * k + h]);
            float fu = -o1, fv = -o2;
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
            {
                const float x = byteF(pk, ch);
                fu = __fmaf_rn(g1[ch], x, fu);
                fv = __fmaf_rn(g2[ch], x, fv);
            }
            // clamping is a projection on a box: it never increases distances either
            fu = fminf(fmaxf(fu, -kBoundLimit16), kBoundLimit16);
            fv = fminf(fmaxf(fv, -kBoundLimit16), kBoundLimit16);
            uu[h] = (int)rintf(fu);
            vv[h] = (int)rintf(fv);
        }
        P.U[k] = ((u32)uu[0] & 0xffffu) | ((u32)uu[1] << 16);
        P.V[k] = ((u32)vv[0] & 0xffffu) | ((u32)vv[1] << 16);
        P.tU = dot2(P.U[k], 0x00010001u, P.tU);
        P.tV = dot2(P.V[k], 0x00010001u, P.tV);
        P.tUU = dot2(P.U[k], P.U[k], P.tUU);
        P.tVV = dot2(P.V[k], P.V[k], P.tVV);
        P.tUV = dot2(P.U[k], P.V[k], P.tUV);
    }
    }
}

struct Sums2D
{
    int n, u, v, uu, vv, uv;
};

// 8-bit grid, the subset given as the byte masks of CvttDeviceTables::subsetByteMask (one 16-byte load instead of four
// nibble -> byte-mask expansions per subset: those were a third of the instructions of a first-tier bound, a quarter-rate
// v_mul_lo_u32 among them)
__device__ __forceinline__ void maskedSumsSel(const Proj2D<true> &P, int n, const uint4 &sel, Sums2D &m)
{
    m.n = n;
    m.u = m.v = m.uu = m.vv = m.uv = 0;
    const u32 s4[4] = {sel.x, sel.y, sel.z, sel.w};
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const u32 um = P.U[k] & s4[k], vm = P.V[k] & s4[k];
        m.u = dot4s(um, 0x01010101u, m.u);
        m.v = dot4s(vm, 0x01010101u, m.v);
        m.uu = dot4s(um, P.U[k], m.uu);
        m.vv = dot4s(vm, P.V[k], m.vv);
        m.uv = dot4s(um, P.V[k], m.uv);
    }
}

template <bool G8>
__device__ __forceinline__ void maskedSums(const Proj2D<G8> &P, u32 mask, Sums2D &m)
{
    m.n = __popc(mask);
    m.u = m.v = m.uu = m.vv = m.uv = 0;
    if constexpr (G8)
    {
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        // four mask bits -> four 0x00 / 0xff bytes
        const u32 bits = (((mask >> (4 * k)) & 0xfu) * 0x00204081u) & 0x01010101u;
        const u32 sel = (bits << 8) - bits;
        const u32 um = P.U[k] & sel, vm = P.V[k] & sel;
        m.u = dot4s(um, 0x01010101u, m.u);
        m.v = dot4s(vm, 0x01010101u, m.v);
        m.uu = dot4s(um, P.U[k], m.uu);
        m.vv = dot4s(vm, P.V[k], m.vv);
        m.uv = dot4s(um, P.V[k], m.uv);
    }
    }
    else
    {
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
        const u32 lo = (u32)__builtin_amdgcn_sbfe(mask, 2 * k, 1);
        const u32 hi = (u32)__builtin_amdgcn_sbfe(mask, 2 * k + 1, 1);
        const u32 sel = (lo & 0x0000ffffu) | (hi & 0xffff0000u);
        const u32 um = P.U[k] & sel, vm = P.V[k] & sel;
        m.u = dot2(um, 0x00010001u, m.u);
        m.v = dot2(vm, 0x00010001u, m.v);
        m.uu = dot2(um, P.U[k], m.uu);
        m.vv = dot2(vm, P.V[k], m.vv);
        m.uv = dot2(um, P.V[k], m.uv);
    }
    }
}

// Lower bound on the error of any trial of the subset with sums `m`.  |coordinates| <= 2040 and
// n <= 16 keep n*sum(uu) and sum(u)^2 below 2^31, so A, B, C are exact; the float steps that
// follow are protected by relative margins on the large terms.
// Straight-line code (no branch, no exec-mask region: 1 024 of these run per wave and stage set):
//   * a subset of fewer than two pixels has a = b = c = 0 exactly, hence lam = L = 0 and lb = 0 (rcpN of an empty subset is
//     0, a finite value);
//   * lam slightly below zero (collinear or single-colour subsets, from the margins) is clamped to 0 ahead of the square root,
//     so no NaN is formed and lb = 0;
//   * for 0 <= L <= n^2 delta^2, where the bound is void, L/n - 2 delta sqrt(L) = s (s/n - 2 delta) with s = sqrt(L) <= n delta
//     is at most -s delta: the two terms differ by a factor of two or more, far beyond any rounding, and the closing max gives 0.
// `rcpN` = 1/n rounded toward zero (kRcpDown, cvtt_kernel_common.h): L * rcpN never exceeds L/n.
template <bool G8 = false>
__device__ __forceinline__ float subsetBound2D(const Sums2D &m, float rcpN, float invScaleSq, float twoDelta)
{
    // |sum u|, |sum v| <= 16 * 2040 fit 24 bits: v_mul_i32_i24 is a full-rate instruction, v_mul_lo_u32 is not; on the 8-bit
    // grid the sums of squares (<= 16 * 128^2) fit as well
    const int a = (G8 ? __mul24(m.n, m.uu) : m.n * m.uu) - __mul24(m.u, m.u);
    const int c = (G8 ? __mul24(m.n, m.vv) : m.n * m.vv) - __mul24(m.v, m.v);
    const int b = (G8 ? __mul24(m.n, m.uv) : m.n * m.uv) - __mul24(m.u, m.v);
    const float fa = (float)a, fc = (float)c, fb = (float)b;
    const float half = (fa + fc) * 0.5f;
    const float diff = (fa - fc) * 0.5f;
    // v_sqrt_f32 is accurate to 1 ulp; the margins below cover that
    const float rad = __builtin_amdgcn_sqrtf(__fmaf_rn(diff, diff, fb * fb));
    const float lam = half * 0.999998f - rad * 1.000002f; // n * scale^2 * (smaller eigenvalue), rounded down
    const float L = fmaxf(lam, 0.0f) * invScaleSq;         // n * R
    const float lb = (L * rcpN - twoDelta * __builtin_amdgcn_sqrtf(L)) * 0.9999f;
    return fmaxf(lb, 0.0f);
}

// =====================================================================================
// The masked sums of the two-subset sets on the 8-bit grid, by the matrix cores (mfma_i8.h).  They are one integer contraction
// with a constant left side,
//   sums[partition][quantity, block] = sum over the 16 pixels of mask[partition][pixel] * feature[pixel][quantity, block],
// and K = 16 of v_mfma_i32_32x32x16_i8 is the pixels of a block.  The masks are the B operand (0 / 1 bytes, 32 partitions per
// tile); the features of four blocks are the 32 rows of the A operand, eight per block: u, v, and uu, vv, uv each as
// lo = x & 127 and hi = x >> 7 (|u|, |v| <= 127, so lo is in [0, 127] and hi in [-127, 126], and the sum is lo + 128 hi summed).
// Rows are ordered so that a lane of the result holds whole blocks: row = (q & 3) | (block & 1) << 2 | (q >> 2) << 3 |
// (block >> 1) << 4 puts quantity q of block 2 j + (lane >> 5) of the group in register 8 j + q.  A lane of the result is one
// partition: its subset sizes and their reciprocals are constants of the tile.
// Per block the wave shares a record of 16 words in LDS: U[4], V[4] of Proj2D<true>, tU tV tUU tVV, tUV, the block's best
// error, its static alpha error, one unused.
// =====================================================================================
constexpr int kT1RecWords = 16;
constexpr int kT1AliveAt = 16 * kT1RecWords; // behind the records: bit p of word [tile][block] = partition 32 tile + p stays

// quantity of A-operand row r, and its block within the group of four
__device__ __forceinline__ constexpr int t1RowQuantity(int r) { return (r & 3) + 4 * ((r >> 3) & 1); }
__device__ __forceinline__ constexpr int t1RowBlock(int r) { return 2 * (r >> 4) + ((r >> 2) & 1); }

// the B operand of tile `tile` for this lane: pixels 8 h .. 8 h + 7 of partition 32 tile + (lane & 31), one 0 / 1 byte each
__device__ __forceinline__ u64 t1MaskOperand(u32 mask16, int h)
{
    const u32 m8 = (mask16 >> (8 * h)) & 0xffu;
    const u32 lo = ((m8 & 0xfu) * 0x00204081u) & 0x01010101u;
    const u32 hi = ((m8 >> 4) * 0x00204081u) & 0x01010101u;
    return (u64)lo | ((u64)hi << 32);
}

// the A operand of a group of four blocks for this lane: quantity q of pixels 8 h .. 8 h + 7 of the lane's block (`rec`)
__device__ __forceinline__ u64 t1FeatureOperand(const u32 *rec, int h, int q)
{
    const uint2 U = *reinterpret_cast<const uint2 *>(rec + 2 * h), V = *reinterpret_cast<const uint2 *>(rec + 4 + 2 * h);
    // q: 0 u, 1 v, 2 3 uu, 4 5 vv, 6 7 uv
    const bool firstV = (q == 1) | (q == 4) | (q == 5), secondU = (q == 2) | (q == 3);
    const u32 a[2] = {firstV ? V.x : U.x, firstV ? V.y : U.y};
    const u32 b[2] = {secondU ? U.x : V.x, secondU ? U.y : V.y};
    const int sh = (q & 1) ? 7 : 0;
    const u32 keep = (q & 1) ? 0xffu : 0x7fu;
    u32 w[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
        u32 acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const int x = __builtin_amdgcn_sbfe((int)a[i], 8 * k, 8), y = __builtin_amdgcn_sbfe((int)b[i], 8 * k, 8);
            acc |= ((u32)(__mul24(x, y) >> sh) & keep) << (8 * k);
        }
        w[i] = (q < 2) ? a[i] : acc;
    }
    return (u64)w[0] | ((u64)w[1] << 32);
}

} // namespace

// bit k of the result = bit 4k + c of m: the partitions sub-lane c of a quad looks after
__device__ __forceinline__ u32 everyFourth(u64 m, int c)
{
    u64 x = (m >> c) & 0x1111111111111111ull;
    x = (x | (x >> 3)) & 0x0303030303030303ull;
    x = (x | (x >> 6)) & 0x000f000f000f000full;
    x = (x | (x >> 12)) & 0x000000ff000000ffull;
    x = (x | (x >> 24)) & 0xffffull;
    return (u32)x;
}
