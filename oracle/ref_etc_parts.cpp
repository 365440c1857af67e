// TEST INFRASTRUCTURE ONLY -- never linked or imported by the product path.
//
// The reference's own small ETC functions over the domains of etc_parts.h, with the entry points of
// cvtt_oracle_etc_parts.inc under the names ref_etc_parts / ref_etc_parts_at.  Compiled together with the reference's
// single-file build (sources stay where they are; see oracle/Makefile) into oracle/_ref/libcvtt_ref_etcparts.so, which is
// git-ignored.  The functions are private statics of cvtt::Internal::ETCComputer: the reference is included with the two
// access keywords defined away, after every standard header it uses has been included under the real ones.
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include <emmintrin.h>
#include <xmmintrin.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <thread>
#include <vector>

#define private public
#define protected public
#include "ConvectionKernels_SingleFile.cpp"
#undef private
#undef protected

#include "etc_parts.h"

namespace
{
    typedef cvtt::Internal::ETCComputer Computer;
    typedef cvtt::ParallelMath PM;
    typedef PM::UInt15 MUInt15;
    typedef PM::Float MFloat;

    struct Sweep
    {
        int part, variant;
        cvtt::Options options;
        const int32_t *table;
    };

    uint32_t be32(const uint8_t *p)
    {
        return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
    }

    // inputs n0 ... n0 + 7, one per lane
    void eval8(const Sweep &s, uint32_t n0, uint32_t out[8])
    {
        switch (s.part)
        {
        case ETCP_RESOLVE_TH:
        {
            MUInt15 q[3], targets[3], granularity;
            for (int lane = 0; lane < 8; lane++)
            {
                int g, t[3], qq[3];
                etcp_th_args(s.table, n0 + lane, &g, t, qq);
                PM::PutUInt15(granularity, lane, (uint16_t)g);
                for (int ch = 0; ch < 3; ch++)
                {
                    PM::PutUInt15(targets[ch], lane, (uint16_t)t[ch]);
                    PM::PutUInt15(q[ch], lane, (uint16_t)qq[ch]);
                }
            }
            Computer::ResolveTHFakeBT709Rounding(q, targets, granularity);
            for (int lane = 0; lane < 8; lane++)
            {
                const int qq[3] = {PM::Extract(q[0], lane), PM::Extract(q[1], lane), PM::Extract(q[2], lane)};
                out[lane] = etcp_pack3(qq, 15);
            }
            return;
        }
        case ETCP_RESOLVE_HALF:
        {
            MUInt15 q[3], cumulative[3];
            for (int ch = 0; ch < 3; ch++)
                q[ch] = PM::MakeUInt15(0);
            for (int lane = 0; lane < 8; lane++)
            {
                int c[3];
                etcp_half_args(s.table, n0 + lane, c);
                for (int ch = 0; ch < 3; ch++)
                    PM::PutUInt15(cumulative[ch], lane, (uint16_t)c[ch]);
            }
            const bool differential = (s.variant & 1) != 0;
            if (s.variant & 2)
                Computer::ResolveHalfBlockFakeBT709RoundingAccurate(q, cumulative, differential);
            else
                Computer::ResolveHalfBlockFakeBT709RoundingFast(q, cumulative, differential);
            for (int lane = 0; lane < 8; lane++)
            {
                const int qq[3] = {PM::Extract(q[0], lane), PM::Extract(q[1], lane), PM::Extract(q[2], lane)};
                out[lane] = etcp_pack3(qq, etcp_half_limit(s.variant));
            }
            return;
        }
        case ETCP_ERR_FAKE:
        case ETCP_ERR_WU:
        case ETCP_ERR2:
        {
            MUInt15 rec[3], px[3];
            MFloat pw[3];
            for (int lane = 0; lane < 8; lane++)
            {
                int r[3], p[3];
                float w[3];
                etcp_err_args(s.table, n0 + lane, r, p, w);
                if (s.part == ETCP_ERR2 && s.variant == 1)
                    etcp_err2_partner(n0 + lane, r);
                for (int ch = 0; ch < 3; ch++)
                {
                    PM::PutUInt15(rec[ch], lane, (uint16_t)r[ch]);
                    PM::PutUInt15(px[ch], lane, (uint16_t)p[ch]);
                    PM::PutFloat(pw[ch], lane, w[ch]);
                }
            }
            MFloat e;
            if (s.part == ETCP_ERR_FAKE)
                e = Computer::ComputeErrorFakeBT709(rec, pw);
            else if (s.part == ETCP_ERR_WU && s.variant == 0)
                e = Computer::ComputeErrorUniform(rec, px);
            else
                e = Computer::ComputeErrorWeighted(rec, pw, s.options);
            for (int lane = 0; lane < 8; lane++)
                out[lane] = etcp_float_bits(PM::Extract(e, lane));
            return;
        }
        case ETCP_PLANAR:
            // the reference has no function of its own for this: the format's bit replication, 6 bits (7 for green) to 8
            for (int lane = 0; lane < 8; lane++)
            {
                const uint32_t n = n0 + lane, coeff = n & 127u, ch = (n >> 7) & 3u;
                out[lane] = ch == 1 ? ((coeff << 1) | (coeff >> 6)) : ((coeff << 2) | (coeff >> 4));
            }
            return;
        case ETCP_EMIT_T:
            for (int lane = 0; lane < 8; lane++)
            {
                etcp_t_args a;
                etcp_t_args_of(n0 + lane, s.variant & 2, etcp_pattern_of(n0 + lane), &a);
                const PM::ScalarUInt16 line[3] = {(PM::ScalarUInt16)a.line[0], (PM::ScalarUInt16)a.line[1], (PM::ScalarUInt16)a.line[2]};
                const PM::ScalarUInt16 iso[3] = {(PM::ScalarUInt16)a.iso[0], (PM::ScalarUInt16)a.iso[1], (PM::ScalarUInt16)a.iso[2]};
                uint8_t bytes[8];
                Computer::EmitTModeBlock(bytes, line, iso, (int32_t)a.selectors, (PM::ScalarUInt16)a.table, a.opaque != 0);
                out[lane] = be32(bytes + 4 * (s.variant & 1));
            }
            return;
        case ETCP_EMIT_H:
            for (int lane = 0; lane < 8; lane++)
            {
                etcp_h_args a;
                etcp_h_args_of(n0 + lane, s.variant & 2, etcp_pattern_of(n0 + lane), &a);
                const PM::ScalarUInt16 bc[2] = {(PM::ScalarUInt16)a.bc[0], (PM::ScalarUInt16)a.bc[1]};
                uint8_t bytes[8];
                Computer::EmitHModeBlock(bytes, bc, (PM::ScalarUInt16)a.sector, (PM::ScalarUInt16)a.sign, (PM::ScalarUInt16)a.table, a.opaque != 0);
                out[lane] = be32(bytes + 4 * (s.variant & 1));
            }
            return;
        }
        for (int lane = 0; lane < 8; lane++)
            out[lane] = 0;
    }

    bool setup(Sweep &s, int part, int variant, const float *weights3, const int32_t *table)
    {
        if (part < 0 || part >= ETCP_PARTS)
            return false;
        s.part = part;
        s.variant = variant;
        s.table = table;
        if (weights3)
        {
            s.options.redWeight = weights3[0];
            s.options.greenWeight = weights3[1];
            s.options.blueWeight = weights3[2];
        }
        return true;
    }

    struct RoundNearest
    {
        unsigned csr;
        RoundNearest() : csr(_mm_getcsr()) { _mm_setcsr((csr & ~_MM_ROUND_MASK) | _MM_ROUND_NEAREST); }
        ~RoundNearest() { _mm_setcsr(csr); }
    };
}

extern "C" int ref_etc_parts(int part, int variant, const float *weights3, const int32_t *table, uint32_t firstChunk, uint32_t numChunks,
                             uint64_t *sums, uint32_t *full, uint64_t *flagged, int threads)
{
    Sweep s;
    if (!setup(s, part, variant, weights3, table) || (uint64_t)firstChunk + numChunks > etcp_chunks(part, variant))
        return -1;
    if (threads < 1) threads = 1;
    if ((uint32_t)threads > numChunks) threads = (int)(numChunks ? numChunks : 1);
    std::vector<uint64_t> flags((size_t)threads, 0);
    auto work = [&](int t) {
        RoundNearest scope;
        const uint32_t begin = firstChunk + (uint32_t)((uint64_t)numChunks * (uint64_t)t / (uint64_t)threads);
        const uint32_t end = firstChunk + (uint32_t)((uint64_t)numChunks * (uint64_t)(t + 1) / (uint64_t)threads);
        uint64_t mine = 0;
        for (uint32_t c = begin; c < end; c++)
        {
            uint64_t acc = 0;
            for (uint32_t k = 0; k < ETCP_CHUNK; k += 8)
            {
                uint32_t r[8];
                eval8(s, c * ETCP_CHUNK + k, r);
                for (uint32_t lane = 0; lane < 8; lane++)
                {
                    acc += etcp_term(r[lane], k + lane);
                    if (s.part <= ETCP_RESOLVE_HALF)
                        mine += r[lane] >> 31;
                    if (full)
                        full[(size_t)(c - firstChunk) * ETCP_CHUNK + k + lane] = r[lane];
                }
            }
            if (sums)
                sums[c - firstChunk] = acc;
        }
        flags[(size_t)t] = mine;
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++)
        pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool)
        th.join();
    uint64_t total = 0;
    for (uint64_t f : flags)
        total += f;
    if (flagged)
        *flagged = total;
    return 0;
}

// each listed input in lane (input & 7) of a call whose other lanes hold its neighbours
extern "C" int ref_etc_parts_at(int part, int variant, const float *weights3, const int32_t *table, const uint32_t *inputs, size_t count, uint32_t *out)
{
    Sweep s;
    if (!setup(s, part, variant, weights3, table))
        return -1;
    const uint64_t limit = (uint64_t)etcp_chunks(part, variant) * ETCP_CHUNK;
    RoundNearest scope;
    for (size_t i = 0; i < count; i++)
    {
        if (inputs[i] >= limit)
            return -1;
        uint32_t r[8];
        eval8(s, inputs[i] & ~7u, r);
        out[i] = r[inputs[i] & 7u];
    }
    return 0;
}
