/* TEST INFRASTRUCTURE ONLY -- the small functions of cvtt_oracle_etc2.inc one at a time, over the domains of etc_parts.h:
 * the resolvers of ETC_UseFakeBT709, the three metrics, planar_decode and the T / H emitters.  Included by cvtt_oracle.c
 * after cvtt_oracle_etc2.inc.  tests/test_etc_primitives_cpu.py holds these equal to the reference's own functions
 * (ref_etc_parts.cpp), tests/test_etc_primitives_gpu.py holds the device functions equal to these. */
#include "etc_parts.h"

typedef struct
{
    int part, variant;
    etc_ctx_t cx;
    const int32_t *table;
} etc_parts_sweep_t;

static uint32_t etc_parts_be32(const uint8_t *p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

static uint32_t etc_parts_eval(const etc_parts_sweep_t *s, uint32_t n)
{
    switch (s->part)
    {
    case ETCP_RESOLVE_TH:
    {
        int g, targets[3], q[3];
        etcp_th_args(s->table, n, &g, targets, q);
        etc_resolve_th_fake(q, targets, g);
        return etcp_pack3(q, 15);
    }
    case ETCP_RESOLVE_HALF:
    {
        int cumulative[3], q[3] = {0, 0, 0};
        etcp_half_args(s->table, n, cumulative);
        etc_resolve_half_fake(&s->cx, q, cumulative, s->variant & 1);
        return etcp_pack3(q, etcp_half_limit(s->variant));
    }
    case ETCP_ERR_FAKE:
    case ETCP_ERR_WU:
    case ETCP_ERR2:
    {
        int rec[3], px[3];
        float pw[3];
        etcp_err_args(s->table, n, rec, px, pw);
        if (s->part == ETCP_ERR_FAKE)
            return etcp_float_bits(etc_error_fake(rec, pw));
        if (s->part == ETCP_ERR2 && s->variant == 1)
            etcp_err2_partner(n, rec);
        return etcp_float_bits(etc_error_wu(&s->cx, rec, px, pw));
    }
    case ETCP_PLANAR:
        return (uint32_t)planar_decode((int)(n & 127u), (int)((n >> 7) & 3u));
    case ETCP_EMIT_T:
    {
        etcp_t_args a;
        uint8_t out[8];
        etcp_t_args_of(n, s->variant & 2, etcp_pattern_of(n), &a);
        etc2_emit_t(out, a.line, a.iso, a.selectors, a.table, a.opaque);
        return etc_parts_be32(out + 4 * (s->variant & 1));
    }
    case ETCP_EMIT_H:
    {
        etcp_h_args a;
        uint8_t out[8];
        etcp_h_args_of(n, s->variant & 2, etcp_pattern_of(n), &a);
        etc2_emit_h(out, a.bc, a.sector, a.sign, a.table, a.opaque);
        return etc_parts_be32(out + 4 * (s->variant & 1));
    }
    }
    return 0;
}

typedef struct
{
    const etc_parts_sweep_t *sweep;
    uint32_t chunkBegin, chunkEnd, firstChunk;
    uint64_t *sums;
    uint32_t *full;
    uint64_t flagged;
} etc_parts_job_t;

static void *etc_parts_main(void *arg)
{
    etc_parts_job_t *j = (etc_parts_job_t *)arg;
    unsigned csr = _mm_getcsr();
    _mm_setcsr((csr & ~_MM_ROUND_MASK) | _MM_ROUND_NEAREST);
    for (uint32_t c = j->chunkBegin; c < j->chunkEnd; c++)
    {
        uint64_t acc = 0;
        for (uint32_t k = 0; k < ETCP_CHUNK; k++)
        {
            const uint32_t r = etc_parts_eval(j->sweep, c * ETCP_CHUNK + k);
            acc += etcp_term(r, k);
            if (j->sweep->part <= ETCP_RESOLVE_HALF)
                j->flagged += r >> 31;
            if (j->full)
                j->full[(size_t)(c - j->firstChunk) * ETCP_CHUNK + k] = r;
        }
        if (j->sums)
            j->sums[c - j->firstChunk] = acc;
    }
    _mm_setcsr(csr);
    return NULL;
}

static int etc_parts_setup(etc_parts_sweep_t *s, int part, int variant, const float *weights3, const int32_t *table)
{
    if (part < 0 || part >= ETCP_PARTS)
        return -1;
    memset(s, 0, sizeof(*s));
    s->part = part;
    s->variant = variant;
    s->table = table;
    s->cx.uniform = part == ETCP_ERR_WU && variant == 0;
    s->cx.fakeAccurate = part == ETCP_RESOLVE_HALF && (variant & 2) != 0;
    if (weights3)
    {
        s->cx.rw = weights3[0];
        s->cx.gw = weights3[1];
        s->cx.bw = weights3[2];
    }
    return 0;
}

/* chunks [firstChunk, firstChunk + numChunks) of a sweep: their checksums into `sums`, their results in full into `full`
 * (either may be NULL), the number of resolver results that carry ETCP_FLAG into `flagged`.  -1: no such part or chunk */
int orc_etc_parts(int part, int variant, const float *weights3, const int32_t *table, uint32_t firstChunk, uint32_t numChunks,
                  uint64_t *sums, uint32_t *full, uint64_t *flagged, int threads)
{
    etc_parts_sweep_t s;
    if (etc_parts_setup(&s, part, variant, weights3, table) != 0)
        return -1;
    if ((uint64_t)firstChunk + numChunks > etcp_chunks(part, variant))
        return -1;
    if (threads < 1) threads = 1;
    if ((uint32_t)threads > numChunks) threads = (int)(numChunks ? numChunks : 1);
    etc_parts_job_t *jobs = (etc_parts_job_t *)calloc((size_t)threads, sizeof(etc_parts_job_t));
    pthread_t *tids = (pthread_t *)calloc((size_t)threads, sizeof(pthread_t));
    for (int t = 0; t < threads; t++)
    {
        jobs[t].sweep = &s;
        jobs[t].firstChunk = firstChunk;
        jobs[t].chunkBegin = firstChunk + (uint32_t)((uint64_t)numChunks * (uint64_t)t / (uint64_t)threads);
        jobs[t].chunkEnd = firstChunk + (uint32_t)((uint64_t)numChunks * (uint64_t)(t + 1) / (uint64_t)threads);
        jobs[t].sums = sums;
        jobs[t].full = full;
    }
    if (threads == 1)
        etc_parts_main(&jobs[0]);
    else
    {
        for (int t = 0; t < threads; t++)
            pthread_create(&tids[t], NULL, etc_parts_main, &jobs[t]);
        for (int t = 0; t < threads; t++)
            pthread_join(tids[t], NULL);
    }
    uint64_t total = 0;
    for (int t = 0; t < threads; t++)
        total += jobs[t].flagged;
    if (flagged)
        *flagged = total;
    free(jobs);
    free(tids);
    return 0;
}

/* the results of the inputs `inputs[0 ... count)` of a sweep, whichever chunks they lie in */
int orc_etc_parts_at(int part, int variant, const float *weights3, const int32_t *table, const uint32_t *inputs, size_t count, uint32_t *out)
{
    etc_parts_sweep_t s;
    if (etc_parts_setup(&s, part, variant, weights3, table) != 0)
        return -1;
    const uint64_t limit = (uint64_t)etcp_chunks(part, variant) * ETCP_CHUNK;
    unsigned csr = _mm_getcsr();
    _mm_setcsr((csr & ~_MM_ROUND_MASK) | _MM_ROUND_NEAREST);
    int rc = 0;
    for (size_t i = 0; i < count && rc == 0; i++)
    {
        if (inputs[i] >= limit)
            rc = -1;
        else
            out[i] = etc_parts_eval(&s, inputs[i]);
    }
    _mm_setcsr(csr);
    return rc;
}
